// Test-split evaluation with prediction maps (test.py: calculate_metrics + the per-image
// create_bin_heat_mask_from_list / save_color_heatmap / overlay_mask_on_image of
// scripts/map_generator.py) as one pass over a batch of logits.  Per pixel p = sigmoid(logit);
//   prob      f32 p
//   heat      u8  floor(clamp(p, 0, 1) * 255 + 0.5)        (torchvision save_image of heat)
//   mask      u8  255 where p > mask_threshold             (binmsk = heat > 0.4)
//   heat_rgb  u8  floor(v * 255 + 0.5), v = clamp((1 - a) image + a lut[min(int(256 p), 255)], 0, 1)
//             with matplotlib's 256-entry green -> yellow -> red table in closed form
//   mask_rgb  u8  the source byte u = floor(255 image + 0.5); where M = p > mask_threshold the
//             truncated blend u (1 - alpha) + color alpha; `color` on the outline band: the
//             pixels whose 3x3 neighbourhood holds both a true and a false M (false outside
//             the image)
//   sums      f64 [B, 12]: the eleven msu_seg_metrics columns at sig_threshold and the
//             BCE-with-logits sum
// A workgroup owns a 64 x 16 tile, a thread 4 consecutive pixels of a row.  The M bits of the
// tile plus a one-pixel halo sit in LDS; a halo pixel's bit comes from the same prob_of() the
// owning tile evaluates, so the outline agrees across tile seams.  Sums: f32 partials per tile
// (<= 1024 pixels: the binary counts are exact), then f64 totals per image in a fixed order.
#include "common.h"

namespace {

constexpr int TW = 64, TH = 16;          // tile
constexpr int MH = TH + 2, MS = TW + 4;  // mask tile rows (halo) and its row stride in bytes
constexpr int NHALO = 2 * (TW + 2) + 2 * TH;
constexpr int NQ = 12;

struct PredArgs {
  const void* logits;
  const float* image;
  const float* label;
  float* prob;
  uint8_t* heat;
  uint8_t* mask;
  uint8_t* heat_rgb;
  uint8_t* mask_rgb;
  float* part;
  int H, W;
  float sig_thr, mask_thr, heat_alpha, mask_alpha;
  uint32_t color;
  int outline;
};

MSU_DEV float prob_of(float x) { return 1.f / (1.f + __expf(-x)); }
MSU_DEV uint32_t quant255(float v) { return (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f + 0.5f); }

// green -> yellow -> red (LinearSegmentedColormap.from_list, N = 256) at index i: t = i / 255,
// R = t <= .5 ? 2t : 1, G = t <= .5 ? g0 + (1 - g0) 2t : 2 - 2t with g0 = 128 / 255, B = 0
// (t <= .5 <=> i <= 127)
MSU_DEV void lut_g2r(int i, float& r, float& g) {
  const float t2 = (float)i * (2.f / 255.f);
  const float g0 = 128.f / 255.f;
  r = i <= 127 ? t2 : 1.f;
  g = i <= 127 ? g0 + (1.f - g0) * t2 : 2.f - t2;
}

// VEC: W % 4 == 0 and every pointer 16-B aligned: 16-B (f32) / 8-B (16-bit) loads, float4,
// packed-byte and 3 x u32 stores; otherwise per-pixel accesses with bounds.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) pred_maps_kernel(PredArgs a) {
  __shared__ uint32_t ms[MH * MS / 4];
  __shared__ float red[4][NQ];
  uint8_t* msb = reinterpret_cast<uint8_t*>(ms);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int H = a.H, W = a.W;
  const long HW = (long)H * W;
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  const int x0 = tx0 + tx * 4, y = ty0 + ty;
  const long pix = (long)y * W + x0;
  const T* lg = (const T*)a.logits + b * HW;
  const bool has_img = a.image != nullptr, has_lab = a.label != nullptr;
  const bool band = a.mask_rgb != nullptr && a.outline != 0;

  bool ok[4];
  float xv[4] = {0.f, 0.f, 0.f, 0.f}, lab[4] = {0.f, 0.f, 0.f, 0.f}, im[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ok[j] = y < H && x0 + j < W;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) im[c][j] = 0.f;
  if (VEC) {
    if (ok[0]) {  // W % 4 == 0: the four pixels are inside together
      Vec4<T>::load(lg + pix, xv);
      if (has_lab) Vec4<float>::load(a.label + b * HW + pix, lab);
      if (has_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Vec4<float>::load(a.image + ((long)b * 3 + c) * HW + pix, im[c]);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!ok[j]) continue;
      xv[j] = to_f32(lg[pix + j]);
      if (has_lab) lab[j] = a.label[b * HW + pix + j];
      if (has_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) im[c][j] = a.image[((long)b * 3 + c) * HW + pix + j];
      }
    }
  }

  // the halo pixel of this thread (threads 0 .. NHALO-1): top row, bottom row, left, right column
  float hx = 0.f;
  bool hok = false;
  int hr = 0, hc = 0;
  if (band && tid < NHALO) {
    if (tid < TW + 2) { hr = 0; hc = tid; }
    else if (tid < 2 * (TW + 2)) { hr = MH - 1; hc = tid - (TW + 2); }
    else if (tid < 2 * (TW + 2) + TH) { hr = tid - 2 * (TW + 2) + 1; hc = 0; }
    else { hr = tid - 2 * (TW + 2) - TH + 1; hc = TW + 1; }
    const int gy = ty0 + hr - 1, gx = tx0 + hc - 1;
    hok = gy >= 0 && gy < H && gx >= 0 && gx < W;
    if (hok) hx = to_f32(lg[(long)gy * W + gx]);
  }

  float p[4];
  uint32_t mk[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[j] = prob_of(xv[j]);
    mk[j] = ok[j] && p[j] > a.mask_thr ? 1u : 0u;
  }

  uint32_t edge[4] = {0u, 0u, 0u, 0u};
  if (band) {
#pragma unroll
    for (int j = 0; j < 4; ++j) msb[(ty + 1) * MS + tx * 4 + 1 + j] = (uint8_t)mk[j];
    if (tid < NHALO) msb[hr * MS + hc] = hok && prob_of(hx) > a.mask_thr ? 1 : 0;
    __syncthreads();
    // columns tx*4 .. tx*4+5 of rows ty .. ty+2 (two aligned words per row); pixel j looks at
    // columns j .. j+2
    uint32_t any[4] = {0u, 0u, 0u, 0u}, all[4] = {1u, 1u, 1u, 1u};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const uint32_t lo = ms[((ty + r) * MS) / 4 + tx], hi = ms[((ty + r) * MS) / 4 + tx + 1];
      const uint64_t w = (uint64_t)lo | ((uint64_t)hi << 32);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint32_t v = (uint32_t)(w >> (8 * (j + k))) & 1u;
          any[j] |= v;
          all[j] &= v;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) edge[j] = any[j] & (all[j] ^ 1u);
  }

  // ---- sums
  if (a.part != nullptr) {
    float acc[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!ok[j]) continue;
      const float pj = p[j], x = xv[j];
      const float pb = pj > a.sig_thr ? 1.f : 0.f;
      acc[1] += pj * pj;
      acc[3] += pj;
      if (has_lab) {
        const float g = lab[j] > 0.f ? 1.f : 0.f;  // ground_truth = label > 0
        acc[0] += pj * g;
        acc[2] += g;
        acc[4] += (1.f - g) * pj;
        acc[5] += g * (1.f - pj);
        acc[6] += (1.f - pj) * (1.f - g);
        acc[7] += pb * g;
        acc[8] += pb * (1.f - g);
        acc[9] += (1.f - pb) * g;
        acc[10] += (1.f - pb) * (1.f - g);
        acc[11] += fmaxf(x, 0.f) - x * g + log1pf(__expf(-fabsf(x)));
      } else {
        acc[8] += pb;  // predicted positives
      }
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const float s = group_sum<64>(acc[k]);
      if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (tid < NQ) {
      const long row = (long)b * (gridDim.x * gridDim.y) + (long)blockIdx.y * gridDim.x + blockIdx.x;
      a.part[row * NQ + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
  }

  // ---- byte planes
  uint32_t hq[4], hrgb[3][4], mrgb[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) hq[j] = quant255(p[j]);
  const bool want_rgb = a.heat_rgb != nullptr || a.mask_rgb != nullptr;
  if (want_rgb) {
    const float ha = a.heat_alpha, hb = 1.f - a.heat_alpha;
    const float w1 = a.mask_alpha, w0 = 1.f - a.mask_alpha;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int i = (int)(p[j] * 256.f);
      i = i > 255 ? 255 : i;
      float l[3];
      lut_g2r(i, l[0], l[1]);
      l[2] = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        hrgb[c][j] = quant255(hb * im[c][j] + ha * l[c]);
        const uint32_t u = (uint32_t)(im[c][j] * 255.f + 0.5f);
        const uint32_t col = (a.color >> (16 - 8 * c)) & 255u;
        // numpy float32: two rounded products, a rounded sum, truncation (astype(uint8))
        const uint32_t mix = (uint32_t)__fadd_rn(__fmul_rn((float)u, w0), __fmul_rn((float)col, w1));
        mrgb[c][j] = edge[j] ? col : (mk[j] ? mix : u);
      }
    }
  }

  const long o = b * HW + pix;
  if (VEC) {
    if (!ok[0]) return;
    if (a.prob != nullptr) Vec4<float>::store(a.prob + o, p);
    if (a.heat != nullptr)
      *reinterpret_cast<uint32_t*>(a.heat + o) = hq[0] | (hq[1] << 8) | (hq[2] << 16) | (hq[3] << 24);
    if (a.mask != nullptr)
      *reinterpret_cast<uint32_t*>(a.mask + o) = (mk[0] | (mk[1] << 8) | (mk[2] << 16) | (mk[3] << 24)) * 255u;
    if (a.heat_rgb != nullptr) {
      uint3 w;
      w.x = hrgb[0][0] | (hrgb[1][0] << 8) | (hrgb[2][0] << 16) | (hrgb[0][1] << 24);
      w.y = hrgb[1][1] | (hrgb[2][1] << 8) | (hrgb[0][2] << 16) | (hrgb[1][2] << 24);
      w.z = hrgb[2][2] | (hrgb[0][3] << 8) | (hrgb[1][3] << 16) | (hrgb[2][3] << 24);
      *reinterpret_cast<uint3*>(a.heat_rgb + 3 * o) = w;
    }
    if (a.mask_rgb != nullptr) {
      uint3 w;
      w.x = mrgb[0][0] | (mrgb[1][0] << 8) | (mrgb[2][0] << 16) | (mrgb[0][1] << 24);
      w.y = mrgb[1][1] | (mrgb[2][1] << 8) | (mrgb[0][2] << 16) | (mrgb[1][2] << 24);
      w.z = mrgb[2][2] | (mrgb[0][3] << 8) | (mrgb[1][3] << 16) | (mrgb[2][3] << 24);
      *reinterpret_cast<uint3*>(a.mask_rgb + 3 * o) = w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!ok[j]) continue;
      if (a.prob != nullptr) a.prob[o + j] = p[j];
      if (a.heat != nullptr) a.heat[o + j] = (uint8_t)hq[j];
      if (a.mask != nullptr) a.mask[o + j] = (uint8_t)(mk[j] * 255u);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (a.heat_rgb != nullptr) a.heat_rgb[3 * (o + j) + c] = (uint8_t)hrgb[c][j];
        if (a.mask_rgb != nullptr) a.mask_rgb[3 * (o + j) + c] = (uint8_t)mrgb[c][j];
      }
    }
  }
}

// one wave per (image, quantity): lanes stride the partial rows, fixed-order double tree
__global__ void __launch_bounds__(256) pred_sums_kernel(const float* part, int B, int nblk, double* out) {
  const int lane = threadIdx.x & 63;
  const int wq = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wq >= B * NQ) return;
  const int b = wq / NQ, q = wq - b * NQ;
  double v = 0.0;
  for (int k = lane; k < nblk; k += 64) v += (double)part[((long)b * nblk + k) * NQ + q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) out[(long)b * NQ + q] = v;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int msu_pred_maps_nblk(int H, int W) {
  if (H <= 0 || W <= 0) return -2;
  const long n = (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  return n > 0x7fffffffL ? -2 : (int)n;
}

int msu_pred_maps(int dtype, const void* logits, const float* image, const float* label, int B, int H, int W,
                  float sig_threshold, float mask_threshold, float heat_alpha, float mask_alpha, int color,
                  int outline, float* prob, unsigned char* heat, unsigned char* mask, unsigned char* heat_rgb,
                  unsigned char* mask_rgb, float* part, double* sums, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0) return -2;
  const int gx = (W + TW - 1) / TW, gy = (H + TH - 1) / TH;
  if (B > 65535 || gy > 65535 || logits == nullptr) return -2;
  if ((heat_rgb != nullptr || mask_rgb != nullptr) && image == nullptr) return -2;  // the overlays blend the image
  if (sums != nullptr && part == nullptr) return -2;
  hipStream_t st = (hipStream_t)stream;
  PredArgs a;
  a.logits = logits;
  a.image = image;
  a.label = label;
  a.prob = prob;
  a.heat = heat;
  a.mask = mask;
  a.heat_rgb = heat_rgb;
  a.mask_rgb = mask_rgb;
  a.part = sums != nullptr ? part : nullptr;
  a.H = H;
  a.W = W;
  a.sig_thr = sig_threshold;
  a.mask_thr = mask_threshold;
  a.heat_alpha = heat_alpha;
  a.mask_alpha = mask_alpha;
  a.color = (uint32_t)color & 0xffffffu;
  a.outline = outline;
  const bool vec = W % 4 == 0 && al16(logits) && al16(image) && al16(label) && al16(prob) && al16(heat) &&
                   al16(mask) && al16(heat_rgb) && al16(mask_rgb);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  if (vec) {
    MSU_DISPATCH(dtype, T, hipLaunchKernelGGL((pred_maps_kernel<T, true>), grid, dim3(256), 0, st, a));
  } else {
    MSU_DISPATCH(dtype, T, hipLaunchKernelGGL((pred_maps_kernel<T, false>), grid, dim3(256), 0, st, a));
  }
  if (sums != nullptr)
    hipLaunchKernelGGL(pred_sums_kernel, dim3((unsigned)((B * NQ + 3) / 4)), dim3(256), 0, st, part, B, gx * gy, sums);
  return MSU_CHECK_LAUNCH();
}

}  // extern "C"
