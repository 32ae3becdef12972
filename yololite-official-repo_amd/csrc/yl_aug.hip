// Training-time augmentation kernel for gfx950: the sibling of yl_pre.hip.  One launch and ONE bilinear gather per
// output pixel turn a packed batch of variable-size uint8 HWC BGR images into the [B,3,S,S] fp32 planar RGB tensor the
// trainable backbone takes.  Replaces, on the training path of the reference, the 4-image mosaic of the dataset
// (scripts/data/dataset.py:124-175: four cv2.resize + paste) and get_base_transform (scripts/data/augment.py:54-101:
// HorizontalFlip, VerticalFlip, Affine, one of RandomBrightnessContrast / HueSaturationValue / RGBShift / ChannelShuffle,
// GaussNoise, LongestMaxSize + PadIfNeeded, Normalize), which run on CPU workers through Albumentations and cv2.
// Every geometric step is folded by the host into one inverse 2x3 map per image (letterbox^-1, affine^-1, un-flip), so a
// pixel is interpolated once where the reference interpolates up to three times; float pixels are never rounded to uint8
// between steps.  Left out: ColorJitter (its contrast term needs the image mean: a second pass), MotionBlur (needs
// neighbouring warped pixels), cutmix.  Only IEEE-exact fp32 operations, each rounded where it is written (compiled with
// -ffp-contract=off), and an integer-only counter hash for the noise: tests/_augment_np.py restates it bit for bit.
// HBM-bound: 12 B written per output pixel, the 4-tap reuse of the sources is absorbed by L2; no LDS, no atomics.
#include "yl_internal.h"
#include <math.h>

static_assert(sizeof(yl_aug_tile) == 32 && sizeof(yl_aug_image) == 96, "descriptor layout is part of the ABI");

__device__ __forceinline__ uint32_t yl_aug_mix(uint32_t h) {     // 32-bit finaliser: xor-shift / odd multiply
  h ^= h >> 16; h *= 0x7feb352du;
  h ^= h >> 15; h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ float yl_aug_clip255(float v) { return fminf(fmaxf(v, 0.0f), 255.0f); }

// RGB (0..255) -> hue in degrees [0,360), saturation [0,1], value (0..255); shifts; back.  colorsys' formulas in fp32.
__device__ __forceinline__ void yl_aug_hsv(float* c, float dh, float ds, float dv) {
  const float r = c[0], g = c[1], b = c[2];
  float v = fmaxf(fmaxf(r, g), b);
  const float mn = fminf(fminf(r, g), b);
  const float d = v - mn;
  float s = 0.0f, h = 0.0f;
  if (d > 0.0f) {
    s = d / v;
    if (v == r) h = 60.0f * ((g - b) / d);
    else if (v == g) h = 120.0f + 60.0f * ((b - r) / d);
    else h = 240.0f + 60.0f * ((r - g) / d);
    if (h < 0.0f) h = h + 360.0f;
  }
  h = h + 2.0f * dh;                                 // OpenCV hue units are half degrees
  if (h < 0.0f) h = h + 360.0f;
  if (h >= 360.0f) h = h - 360.0f;
  s = fminf(fmaxf(s + ds / 255.0f, 0.0f), 1.0f);
  v = yl_aug_clip255(v + dv);
  const float hp = h / 60.0f;
  const float fi = floorf(hp);
  const float f = hp - fi;
  const float p = v * (1.0f - s);
  const float q = v * (1.0f - s * f);
  const float t = v * (1.0f - s * (1.0f - f));
  const int i = (int)fi;
  if (i == 0) { c[0] = v; c[1] = t; c[2] = p; }
  else if (i == 1) { c[0] = q; c[1] = v; c[2] = p; }
  else if (i == 2) { c[0] = p; c[1] = v; c[2] = t; }
  else if (i == 3) { c[0] = p; c[1] = q; c[2] = v; }
  else if (i == 4) { c[0] = t; c[1] = p; c[2] = v; }
  else { c[0] = v; c[1] = p; c[2] = q; }
}

__global__ __launch_bounds__(256) void yl_augment_kernel(const unsigned char* __restrict__ src,
                                                         const yl_aug_tile* __restrict__ tiles,
                                                         const yl_aug_image* __restrict__ imgs, int S,
                                                         float* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (x >= S || y >= S) return;
  const yl_aug_image im = imgs[b];
  float c[3] = {114.0f, 114.0f, 114.0f};             // output channel order (R,G,B after the permutation)
  const int ry = y - im.top, rx = x - im.left;
  if (ry >= 0 && ry < im.nh && rx >= 0 && rx < im.nw) {              // inside the letterbox: everything below applies
    const float xf = (float)x, yf = (float)y;
    const float u = (im.m[0] * xf + im.m[1] * yf) + im.m[2];         // frame coordinates, pixel centres at +0.5
    const float v = (im.m[3] * xf + im.m[4] * yf) + im.m[5];
    if (u >= 0.0f && u < (float)im.frame_w && v >= 0.0f && v < (float)im.frame_h) {   // false for NaN: border
      for (int k = 0; k < im.num_tiles; ++k) {
        const yl_aug_tile t = tiles[im.first_tile + k];
        if (!(u >= t.x0 && u < t.x1 && v >= t.y0 && v < t.y1)) continue;
        const float sx = (float)t.w0 / (t.x1 - t.x0), sy = (float)t.h0 / (t.y1 - t.y0);
        const float fx = (u - t.x0) * sx - 0.5f, fy = (v - t.y0) * sy - 0.5f;
        const float flx = floorf(fx), fly = floorf(fy);
        const float ax = fx - flx, ay = fy - fly;
        const int ix = (int)flx, iy = (int)fly;
        const int x0 = min(max(ix, 0), t.w0 - 1), x1 = min(max(ix + 1, 0), t.w0 - 1);   // each tile replicates its own edge
        const int y0 = min(max(iy, 0), t.h0 - 1), y1 = min(max(iy + 1, 0), t.h0 - 1);
        const unsigned char* r0 = src + t.offset + (size_t)y0 * t.w0 * 3;
        const unsigned char* r1 = src + t.offset + (size_t)y1 * t.w0 * 3;
        float bgr[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float p00 = (float)r0[x0 * 3 + ch], p01 = (float)r0[x1 * 3 + ch];
          const float p10 = (float)r1[x0 * 3 + ch], p11 = (float)r1[x1 * 3 + ch];
          const float h0 = p00 + (p01 - p00) * ax;
          const float h1 = p10 + (p11 - p10) * ax;
          bgr[ch] = h0 + (h1 - h0) * ay;
        }
        const float rgb[3] = {bgr[2], bgr[1], bgr[0]};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int pc = im.perm[ch];
          c[ch] = pc == 0 ? rgb[0] : (pc == 1 ? rgb[1] : rgb[2]);
        }
        break;
      }
    }
    if (im.color_mode == YL_AUG_BRIGHTNESS_CONTRAST) {
      const float beta = im.color[1] * 255.0f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = yl_aug_clip255(im.color[0] * c[ch] + beta);
    } else if (im.color_mode == YL_AUG_HSV_SHIFT) {
      yl_aug_hsv(c, im.color[0], im.color[1], im.color[2]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = yl_aug_clip255(c[ch]);
    } else if (im.color_mode == YL_AUG_RGB_SHIFT) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = yl_aug_clip255(c[ch] + im.color[ch]);
    }
    if (im.noise_sigma > 0.0f) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        uint32_t key = yl_aug_mix(im.noise_seed ^ yl_aug_mix((uint32_t)y * 0x9E3779B1u + (uint32_t)ch));
        key = yl_aug_mix(key ^ ((uint32_t)x * 0x85EBCA77u));
        uint32_t sum = 0;                                            // twelve 24-bit uniforms: the sum fits 28 bits
        for (uint32_t k = 0; k < 12u; ++k) sum += yl_aug_mix(key + k * 0xC2B2AE3Du) >> 8;
        const float n = (float)sum * (1.0f / 16777216.0f) - 6.0f;    // one rounding in the conversion, then exact scale
        c[ch] = yl_aug_clip255(c[ch] + im.noise_sigma * n);
      }
    }
  }
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const size_t plane = (size_t)S * S;
  float* o = out + (size_t)b * 3 * plane + (size_t)y * S + x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {                                   // A.Normalize's arithmetic, as yl_pre.hip's norm_mode 1
    const float m255 = mean[ch] * 255.0f;
    const float d = 1.0f / (stdv[ch] * 255.0f);
    o[ch * plane] = (c[ch] - m255) * d;
  }
}

extern "C" yl_status yl_augment(const uint8_t* packed_u8_dev, const yl_aug_tile* tiles_dev, const yl_aug_image* imgs_dev,
                                int32_t batch, int32_t size, float* x_dev, void* stream) {
  if (!packed_u8_dev || !tiles_dev || !imgs_dev || !x_dev) return YL_ERR_INVALID;
  if (batch <= 0 || size <= 0 || batch > 65535) return YL_ERR_INVALID;          // batch is the grid's z extent
  dim3 grid((size + 63) / 64, (size + 3) / 4, batch);
  if (grid.y > 65535u) return YL_ERR_INVALID;
  hipLaunchKernelGGL(yl_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed_u8_dev, tiles_dev, imgs_dev,
                     (int)size, x_dev);
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}
