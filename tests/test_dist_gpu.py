"""bench.py under torch.distributed.run with ONE rank on the GPU box: exercises the RCCL (nccl backend)
initialisation and the all-gather code path the 8-GPU driver run uses (world_size 1 is the only size a
1-GPU box can host; the world-2 logic is covered on CPU with gloo in test_host_cpu.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_under_torchrun_one_rank():
    env = dict(os.environ, YL_BENCH_FORCE_COLLECTIVE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29731", os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--no-cpu-baseline", "--full"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1 and d["value"] > 0 and "roofline" in d
    # what the first multi-GPU run reports about itself: ranks in the communicator, per-rank step
    # time, the exchange's own HIP-event time; every timed block is exactly --steps steps
    assert d["rccl_ranks"] == 1 and len(d["ms_per_step_per_rank"]) == 1 and d["allgather_ms"] > 0
    assert d["allgather_bytes_per_rank"] == (8 * 1024 * 6 + 8) * 4
    assert d["blocks"]["steps_each"] == 3 and d["blocks"]["n"] >= 1
    assert d["blocks"]["images_per_sec_min"] <= d["value"] <= d["blocks"]["images_per_sec_max"]


def test_throughput_next_to_an_initialised_process_group_is_within_3_percent():
    """GPU_MAX_HW_QUEUES is load-bearing (a chunk stream that shares a hardware queue with the
    caller's stream serialises the chunks: -25 % once RCCL has created its streams) and used to be set by bench.py and
    the CLIs only.  A host that imports torch FIRST, initialises the nccl process group, and only then imports the
    package must see the same edge_n B=64 throughput as the same host without RCCL (the package default does it)."""
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    res = {}
    for rccl in (0, 1, 0, 1):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_queue_probe.py"), "--rccl", str(rccl)],
                           capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["GPU_MAX_HW_QUEUES"] == "8"
        res.setdefault(rccl, []).append(d["images_per_sec"])
    plain, with_rccl = max(res[0]), max(res[1])
    print(f"images/s without RCCL {res[0]}, with an initialised process group {res[1]}")
    assert with_rccl >= 0.97 * plain, res


def test_c_abi_allgather_dets_with_a_raw_rccl_communicator():
    """yl_allgather_dets with an ncclComm_t created directly on RCCL (world 1 is what a 1-GPU box can
    host): yl_predict writes [dets | counts] into the flat row, the C entry point exchanges it."""
    import ctypes as C
    import glob
    import numpy as np
    import torch
    import yololite_amd as ya
    from yololite_amd import _lib
    from yololite_amd.program import synth_state_dict, zoo_meta
    cands = glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so*")) + ["/opt/rocm/lib/librccl.so"]
    rccl = C.CDLL([c for c in cands if os.path.exists(c)][0], mode=C.RTLD_GLOBAL)

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]
    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    meta = zoo_meta("edge_n", 80, 128)
    m = ya.build_model_from_meta(meta)
    m.load_state_dict(synth_state_dict(meta, seed=2, head_noise=2.0))
    m.to("cuda:0")
    ctx = m._ctx_for(128)
    b, max_out = 4, 64
    x = torch.randn(b, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    row = b * max_out * 6 + b
    local = torch.zeros(row, device="cuda", dtype=torch.float32)
    dets = local[:b * max_out * 6].view(b, max_out, 6)
    counts = local[b * max_out * 6:].view(torch.int32)
    ctx.predict(x, _lib.POST_MAIN, 0.05, 0.5, per_class_cap=300, max_out=max_out, out=(dets, counts))
    allb = torch.full((1, row), -1.0, device="cuda", dtype=torch.float32)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.yl_allgather_dets(ctx.handle, comm, local.data_ptr(), row, allb.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(counts.sum()) > 0 and torch.equal(allb[0].view(torch.int32), local.view(torch.int32))
    assert lib.yl_allgather_dets(ctx.handle, None, local.data_ptr(), row, allb.data_ptr(), st) == -1      # NULL communicator
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    rccl.ncclCommDestroy(comm)


def test_pipelined_gatherer_under_graph_replay_is_self_validating():
    """the path the 8-GPU run takes -- yl_predict writing into DetGatherer's alternating slots
    under hipGraph replay (cache of 4 graphs), ONE asynchronous all-gather per step, results read one step late --
    driven for 60 steps at world 1 with the collective forced; EVERY step's gathered rows must equal the rows of a
    plain (non-pipelined, eager) run of the same input."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import bench
    from yololite_amd import _lib, dist as ydist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29741")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        wl = bench.build_workload("edge_n", 320, 8, seed=1, dev="cuda:0")
        ctx = wl["ctx"]
        xs = [bench.synth_images(8, 320, seed=100 + k).cuda() for k in range(3)]      # three inputs in rotation
        mo = 256
        ctx.set_option("graph", 0); ctx.set_option("streams", 1)
        ref = []
        for x in xs:
            d, c = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
            ref.append((d.clone(), c.clone()))
        assert min(int(c.min()) for _, c in ref) > 0
        ctx.set_option("graph", 1); ctx.set_option("streams", 2)
        gat = ydist.DetGatherer(8, mo, torch.device("cuda", 0))
        steps, checked = 60, 0
        for k in range(steps + 1):
            if k < steps:
                ctx.predict(xs[k % 3], _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo, out=(gat.dets, gat.counts))
                prev = gat.gather()                                 # the PREVIOUS step's result (None on the first)
            else:
                prev = gat.flush()
            if prev is None:
                continue
            d, c = prev                                             # [world, b, max_out, 6], [world, b]
            rd, rc = ref[(k - 1) % 3]
            torch.cuda.synchronize()
            assert torch.equal(c[0], rc), k
            for b in range(8):
                n = int(rc[b])
                assert torch.equal(d[0, b, :n], rd[b, :n]), (k, b)
            checked += 1
        assert checked == steps
    finally:
        dist.destroy_process_group()
