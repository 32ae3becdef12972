"""Host side of the fused training step (yololite_amd.trainops): chunk planner, EMA decay schedule, refusals that
need no device, and the state_dict packing.  No HIP compute here."""
import math

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import trainops

COUNTS = [1, 3, 4, 5, 255, 256, 257, 1023, 4097, 70001]


@pytest.mark.parametrize("chunk", [1024, 4096])
def test_chunk_planner_covers_every_element_once_in_table_order(chunk):
    chunks = trainops.plan_chunks(COUNTS, chunk)
    assert chunks == sorted(chunks, key=lambda c: (c[0], c[1])), "chunks leave table order"
    for s, n in enumerate(COUNTS):
        hit = np.zeros(n, np.int32)
        for seg, off, ln in chunks:
            if seg == s:
                assert 0 <= off and 1 <= ln <= chunk and off + ln <= n and off % 4 == 0
                hit[off:off + ln] += 1
        assert (hit == 1).all(), f"segment {s}: an element is covered {hit.min()}..{hit.max()} times"
    assert len(chunks) == sum(-(-n // chunk) for n in COUNTS)
    assert {c[0] for c in chunks} == set(range(len(COUNTS)))


def test_chunk_planner_edge_cases():
    assert trainops.plan_chunks([], 1024) == []
    assert trainops.plan_chunks([0, 5, 0], 4) == [(1, 0, 4), (1, 4, 1)]
    for bad in (0, 3, 6, -4):
        with pytest.raises(ya.YoloLiteHipError):
            trainops.plan_chunks([8], bad)
    with pytest.raises(ya.YoloLiteHipError):
        trainops.plan_chunks([-1], 4)


@pytest.mark.parametrize("total", [100, 10000])
def test_ema_decay_schedule_is_the_references(total):
    limit = max(100, total // 5)
    assert trainops.ema_warmup_limit(total) == limit
    for u in range(1, 301):
        assert trainops.ema_decay_at(u, 0.999, total) == 0.999 * (1 - math.exp(-u / limit))


def test_cpu_tensors_raise():
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        ya.FusedTrainStep([p])
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        ya.FusedTrainStep([{"params": [p], "lr": 1e-3}], optimizer="sgd", model={"p": p.detach()},
                          ema_model={"p": torch.zeros(8)})


def test_unsupported_tensors_are_refused_before_any_device_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(trainops._lib, "load", boom)
    with pytest.raises(ya.YoloLiteHipError, match="float16"):
        ya.FusedTrainStep([torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))])
    with pytest.raises(ya.YoloLiteHipError, match="non-contiguous"):
        ya.FusedTrainStep([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ya.YoloLiteHipError, match="float16"):
        ya.FusedTrainStep([torch.zeros(8)], model={"p": torch.zeros(8), "b": torch.zeros(3, dtype=torch.float16)},
                          ema_model={"p": torch.zeros(8), "b": torch.zeros(3, dtype=torch.float16)})
    with pytest.raises(ValueError):
        ya.FusedTrainStep([torch.zeros(8)], optimizer="lion")


@pytest.mark.parametrize("kind", ["adamw", "adam", "sgd"])
def test_state_dict_round_trip(kind):
    rs = np.random.RandomState(3)
    n = [5, 1, 7]
    s0 = [torch.from_numpy(rs.randn(k).astype(np.float32)) for k in n]
    s1 = [torch.from_numpy(rs.rand(k).astype(np.float32)) if kind != "sgd" else None for k in n]
    groups = [{"params": [0, 1], "lr": 1e-3, "weight_decay": 0.01}, {"params": [2], "lr": 5e-4, "weight_decay": 0.0}]
    sd = trainops.build_state_dict(kind, groups, [3.0, 0.0, 2.0], s0, s1, 32768.0, 7, 41)
    names = ("exp_avg", "exp_avg_sq") if kind != "sgd" else ("momentum_buffer",)
    assert sorted(sd["state"]) == [0, 2], "a parameter that never stepped has no entry"
    assert set(sd["state"][0]) == {"step", *names}
    assert set(sd["scaler"]) == {"scale", "_growth_tracker"} and sd["ema_updates"] == 41
    steps, tensors, opts, scale, tracker, updates = trainops.parse_state_dict(sd, kind, 3)
    assert steps.tolist() == [3.0, 0.0, 2.0] and (scale, tracker, updates) == (32768.0, 7, 41)
    assert opts == [{"lr": 1e-3, "weight_decay": 0.01}, {"lr": 5e-4, "weight_decay": 0.0}]
    for i in (0, 2):
        assert torch.equal(tensors[i][0], s0[i])
        assert tensors[i][1] is None if kind == "sgd" else torch.equal(tensors[i][1], s1[i])
    s0b = [tensors[i][0] if i in tensors else torch.zeros(n[i]) for i in range(3)]
    s1b = [tensors[i][1] if i in tensors else (None if kind == "sgd" else torch.zeros(n[i])) for i in range(3)]
    again = trainops.build_state_dict(kind, groups, steps, s0b, s1b, scale, tracker, updates)
    assert again.keys() == sd.keys() and again["param_groups"] == sd["param_groups"]
    assert again["scaler"] == sd["scaler"] and sorted(again["state"]) == sorted(sd["state"])
    for i in sd["state"]:
        for k in sd["state"][i]:
            assert torch.equal(again["state"][i][k], sd["state"][i][k])
    with pytest.raises(ValueError):
        trainops.parse_state_dict(sd, "sgd" if kind != "sgd" else "adam", 3)
    with pytest.raises(ValueError):
        trainops.parse_state_dict(sd, kind, 2)
