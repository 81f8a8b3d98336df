// Threshold sweep of the binary validation counts in one pass over the logits: per image and
// class g = label > 0, a histogram of "how many of the K ascending thresholds lie below p",
// p = sigmoid(logit) exactly as metrics.hip forms it.  hist[b][g][j] = pixels of image b in
// class g with t_0 .. t_{j-1} < p (and t_j >= p); the confusion counts of every threshold are
// suffix sums of that row (validation.sweep_counts), so one launch replaces K msu_seg_metrics
// calls.  The predicate is the metrics kernel's, strict: a tie is not positive, a NaN logit is
// positive nowhere (every "t < p" is false: bin 0), +-inf give p = 1 / p = 0.
//
// Work per pixel is the search, not the 6-8 bytes of traffic.  Real images put every pixel
// below t_0 and confident fakes put theirs below t_0 or above t_{K-1}: the two end bins of both
// classes are per-thread registers (two compares against t_0 and t_{K-1}, held in registers),
// reduced once per wave at the end.  Only interior pixels take the branch-free lower bound over
// the thresholds in LDS (ceil(log2 K) steps over t_0 .. t_{K-2}; a wave with no interior lane
// skips it) and one LDS atomic on the block's u32 histogram.  A block then adds its non-zero
// bins to the int64 output with 64-bit integer atomics, after an in-stream clear: integer sums
// do not depend on the arrival order, so the result is bitwise reproducible.
#include "common.h"

namespace {

constexpr int SWEEP_MAX_K = 1024;
constexpr int SWEEP_MAX_BLK = 1024;            // blocks per image
constexpr long SWEEP_MAX_N = 1L << 41;         // a block's share stays below 2^32 (u32 bins)
constexpr int SWEEP_PER_BLOCK = 4096;          // pixels a block takes before the grid is capped

// logits per 16-byte load
template <typename T> struct SweepLoad;
template <> struct SweepLoad<float> {
  static constexpr int V = 4;
  static MSU_DEV void load(const float* p, float (&v)[4]) { Vec4<float>::load(p, v); }
};
template <typename T> struct SweepLoad16 {
  static constexpr int V = 8;
  static MSU_DEV void load(const T* p, float (&v)[8]) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = Fmt16<T>::lo(q[k]);
      v[2 * k + 1] = Fmt16<T>::hi(q[k]);
    }
  }
};
template <> struct SweepLoad<bf16_t> : SweepLoad16<bf16_t> {};
template <> struct SweepLoad<f16_t> : SweepLoad16<f16_t> {};

struct SweepCtx {
  const float* thr;  // LDS: t_0 .. t_{K-2}, +inf up to index half * 2 - 2
  uint32_t* bins;    // LDS: [2][K + 1]
  int K, half;       // half = P2 / 2, P2 the smallest power of two >= K
  float t0, tl;      // t_0, t_{K-1}
};

// e: end-bin counts {g = 0 bin 0, g = 0 bin K, g = 1 bin 0, g = 1 bin K}
MSU_DEV void sweep_pixel(const SweepCtx& c, float x, float lab, uint32_t (&e)[4]) {
  const float p = 1.f / (1.f + __expf(-x));  // metrics.hip's expression
  const bool g = lab > 0.f;
  const bool lo = !(c.t0 < p);  // below every threshold (NaN: no "t < p" holds)
  const bool hi = c.tl < p;     // above every threshold
  e[0] += (uint32_t)(lo && !g);
  e[1] += (uint32_t)(hi && !g);
  e[2] += (uint32_t)(lo && g);
  e[3] += (uint32_t)(hi && g);
  if (!lo && !hi) {  // t_0 < p <= t_{K-1}: count of t_j < p among t_0 .. t_{K-2}, in 1 .. K-1
    int pos = 0;
    for (int s = c.half; s > 0; s >>= 1) pos += c.thr[pos + s - 1] < p ? s : 0;
    atomicAdd(c.bins + (g ? c.K + 1 : 0) + pos, 1u);
  }
}

__global__ void __launch_bounds__(256) sweep_clear_kernel(unsigned long long* hist, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0ull;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) sweep_kernel(const T* logits, const float* label, long N, int nblk,
                                                    const float* thresholds, int K, int half,
                                                    unsigned long long* hist) {
  __shared__ float sthr[SWEEP_MAX_K];
  __shared__ uint32_t sbin[2 * (SWEEP_MAX_K + 1)];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nbin = 2 * (K + 1);
  // the search reads indices 0 .. 2 * half - 2 <= SWEEP_MAX_K - 2
  for (int i = tid; i < SWEEP_MAX_K; i += 256) sthr[i] = i < K - 1 ? thresholds[i] : __builtin_inff();
  for (int i = tid; i < nbin; i += 256) sbin[i] = 0u;
  SweepCtx c;
  c.thr = sthr;
  c.bins = sbin;
  c.K = K;
  c.half = half;
  c.t0 = thresholds[0];
  c.tl = thresholds[K - 1];
  __syncthreads();

  const T* x = logits + (long)b * N;
  const float* t = label + (long)b * N;
  uint32_t e[4] = {0u, 0u, 0u, 0u};
  if (VEC) {
    constexpr int V = SweepLoad<T>::V;
    const long nv = N / V;  // N % V == 0 on this path
    for (long i = (long)blockIdx.x * 256 + tid; i < nv; i += (long)nblk * 256) {
      float xv[V], lv[V];
      SweepLoad<T>::load(x + i * V, xv);
#pragma unroll
      for (int k = 0; k < V; k += 4) {
        float l4[4];
        Vec4<float>::load(t + i * V + k, l4);
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[k + j] = l4[j];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) sweep_pixel(c, xv[k], lv[k], e);
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + tid; i < N; i += (long)nblk * 256)
      sweep_pixel(c, to_f32(x[i]), t[i], e);
  }

  // end bins: one LDS add per wave and bin
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t s = e[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
    // K == 1: bins 0 and K are the whole row
    if ((tid & 63) == 0 && s != 0u) atomicAdd(sbin + (k >> 1) * (K + 1) + ((k & 1) ? K : 0), s);
  }
  __syncthreads();
  unsigned long long* out = hist + (long)b * nbin;
  for (int i = tid; i < nbin; i += 256) {
    const uint32_t v = sbin[i];
    if (v != 0u) atomicAdd(out + i, (unsigned long long)v);
  }
}

inline bool sweep_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int msu_seg_sweep_max_k() { return SWEEP_MAX_K; }

long msu_seg_sweep_max_n() { return SWEEP_MAX_N; }

// logits [B, N] (f32, bf16 or f16), label [B, N] f32, thresholds [K] f32 strictly ascending
// (device); hist [B, 2, K + 1] int64 (device), fully overwritten.
int msu_seg_sweep(int dtype, const void* logits, const float* label, int B, long N, const float* thresholds,
                  int K, long long* hist, void* stream) {
  if (B <= 0 || B > 65535 || N <= 0 || N > SWEEP_MAX_N || K < 1 || K > SWEEP_MAX_K) return -2;
  if (dtype < MSU_F32 || dtype > MSU_F16) return -2;
  if (logits == nullptr || label == nullptr || thresholds == nullptr || hist == nullptr) return -2;
  hipStream_t st = (hipStream_t)stream;
  long nb = (N + SWEEP_PER_BLOCK - 1) / SWEEP_PER_BLOCK;
  const int nblk = (int)(nb > SWEEP_MAX_BLK ? SWEEP_MAX_BLK : nb);
  int p2 = 1;
  while (p2 < K) p2 <<= 1;
  const long nhist = (long)B * 2 * (K + 1);
  unsigned long long* out = (unsigned long long*)hist;
  hipLaunchKernelGGL(sweep_clear_kernel, dim3((unsigned)((nhist + 255) / 256)), dim3(256), 0, st, out, nhist);
  const int V = dtype == MSU_F32 ? 4 : 8;
  const bool vec = N % V == 0 && sweep_al16(logits) && sweep_al16(label);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (vec) {
    MSU_DISPATCH(dtype, T, hipLaunchKernelGGL((sweep_kernel<T, true>), grid, dim3(256), 0, st, (const T*)logits,
                                              label, N, nblk, thresholds, K, p2 / 2, out));
  } else {
    MSU_DISPATCH(dtype, T, hipLaunchKernelGGL((sweep_kernel<T, false>), grid, dim3(256), 0, st, (const T*)logits,
                                              label, N, nblk, thresholds, K, p2 / 2, out));
  }
  return MSU_CHECK_LAUNCH();
}

}  // extern "C"
