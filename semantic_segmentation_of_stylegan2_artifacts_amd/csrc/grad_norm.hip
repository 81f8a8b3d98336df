// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) for the device-side step: the
// sum of squares of the two flat f32 gradient buffers in the pass that also is the step's
// non-finite check (one read, in the place of msu_nonfinite2), and a one-workgroup launch that
// turns it into the gradient norm and folds the clip coefficient into the factor AdamW multiplies
// every gradient by.  Everything is summed in f64 in a fixed order: the square of an f32 is exact
// in f64 (24 + 24 significand bits, exponent within +-300), so 1e-30 and 1e+25 gradients give a
// finite, correct norm, no atomics are needed and two launches agree bitwise.  HBM-bound: one
// 16-byte load per lane where the address allows, four independent loads in flight per lane.
#include "common.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAX_BLOCKS = 1024;  // partial sums: the final reduction is one workgroup

// sum of v over the workgroup's 256 threads, the same tree every time (sh: 256 doubles)
MSU_DEV double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = GN_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

MSU_DEV double sq(double a, float x) { return a + (double)x * (double)x; }
MSU_DEV double sq4(double a, f32x4 q) { return sq(sq(sq(sq(a, q.x), q.y), q.z), q.w); }

// elements of x[0:n] in front of the first 16-byte boundary (all of them when n is smaller)
MSU_DEV int head_len(const float* x, long n) {
  const long h = (4 - (long)(((uintptr_t)x >> 2) & 3)) & 3;
  return (int)(h < n ? h : n);
}

// part[b] = sum of (double)x^2 over workgroup b's share of [x0 | x1].  Each buffer is a scalar
// head (<= 3 elements up to its first 16-byte boundary), a body of 16-byte vectors and a scalar
// tail (<= 3): the vectors of both bodies are one index space walked grid-stride, the <= 12
// scalars go to workgroup 0, one per thread.  A workgroup without elements writes 0.  A
// non-finite element makes its workgroup's sum non-finite and nothing brings it back (x^2 is
// never -inf, and every finite square is far below the f64 range): that sum is the check.
__global__ void __launch_bounds__(GN_THREADS) grad_sumsq2_kernel(const float* x0, long n0, const float* x1,
                                                                 long n1, double* part, float* flag) {
  __shared__ double sh[GN_THREADS];
  const int h0 = head_len(x0, n0), h1 = head_len(x1, n1);
  const f32x4* b0 = (const f32x4*)(x0 + h0);
  const f32x4* b1 = (const f32x4*)(x1 + h1);
  const long v0 = (n0 - h0) >> 2, v1 = (n1 - h1) >> 2, V = v0 + v1;
  const long stride = (long)gridDim.x * GN_THREADS;
  long j = (long)blockIdx.x * GN_THREADS + threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (; j + 3 * stride < V; j += 4 * stride) {
    const long j1 = j + stride, j2 = j + 2 * stride, j3 = j + 3 * stride;
    const f32x4 q0 = j < v0 ? b0[j] : b1[j - v0];
    const f32x4 q1 = j1 < v0 ? b0[j1] : b1[j1 - v0];
    const f32x4 q2 = j2 < v0 ? b0[j2] : b1[j2 - v0];
    const f32x4 q3 = j3 < v0 ? b0[j3] : b1[j3 - v0];
    a0 = sq4(a0, q0);
    a1 = sq4(a1, q1);
    a2 = sq4(a2, q2);
    a3 = sq4(a3, q3);
  }
  for (; j < V; j += stride) a0 = sq4(a0, j < v0 ? b0[j] : b1[j - v0]);
  double acc = (a0 + a1) + (a2 + a3);
  if (blockIdx.x == 0 && threadIdx.x < 12) {
    // threads 0-5: x0's head (0-2) and tail (3-5); threads 6-11: x1's
    const bool second = threadIdx.x >= 6;
    const float* x = second ? x1 : x0;
    const long n = second ? n1 : n0;
    const int h = second ? h1 : h0;
    const long body_end = h + 4 * (second ? v1 : v0);
    const int u = (int)threadIdx.x - (second ? 6 : 0);
    if (u < 3) {
      if (u < h) acc = sq(acc, x[u]);
    } else if (body_end + (u - 3) < n) {
      acc = sq(acc, x[body_end + (u - 3)]);
    }
  }
  const double total = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = total;
    if (flag != nullptr && !isfinite(total)) flag[0] = 1.f;
  }
}

// S = sum of part in a fixed order, then clip_grad_norm_'s rule on the factor AdamW unscales by;
// every step one IEEE double operation, each output rounded to f32 once (one workgroup)
__global__ void __launch_bounds__(GN_THREADS) grad_clip_scale_kernel(const double* part, int nblk,
                                                                     const float* inv_in, double max_norm,
                                                                     float* norm_out, float* inv_out) {
#pragma clang fp contract(off)
  __shared__ double sh[GN_THREADS];
  double a = 0.0;
  for (int i = threadIdx.x; i < nblk; i += GN_THREADS) a += part[i];
  const double S = block_sum(a, sh);
  if (threadIdx.x != 0) return;
  const double inv = inv_in ? (double)inv_in[0] : 1.0;
  const double norm = sqrt(S) * inv;
  const double coef = max_norm / (norm + 1e-6);
  norm_out[0] = (float)norm;
  inv_out[0] = (float)(inv * (coef < 1.0 ? coef : 1.0));  // a NaN coef leaves inv as it is
}

}  // namespace

extern "C" {

int msu_grad_sumsq_nblk(long n) {
  long nb = (n + 4 * GN_THREADS - 1) / (4 * GN_THREADS);
  if (nb > GN_MAX_BLOCKS) nb = GN_MAX_BLOCKS;
  return (int)(nb < 1 ? 1 : nb);
}

int msu_grad_sumsq2(const float* x0, long n0, const float* x1, long n1, double* part, int nblk, float* flag,
                    void* stream) {
  if (part == nullptr || n0 < 0 || n1 < 0 || (x0 == nullptr && n0 > 0) || (x1 == nullptr && n1 > 0) ||
      nblk != msu_grad_sumsq_nblk(n0 + n1))
    return -2;
  hipLaunchKernelGGL(grad_sumsq2_kernel, dim3(nblk), dim3(GN_THREADS), 0, (hipStream_t)stream, x0, n0, x1, n1,
                     part, flag);
  return MSU_CHECK_LAUNCH();
}

int msu_grad_clip_scale(const double* part, int nblk, const float* inv_in, double max_norm, float* norm_out,
                        float* inv_out, void* stream) {
  if (part == nullptr || nblk < 1 || nblk > GN_MAX_BLOCKS || norm_out == nullptr || inv_out == nullptr ||
      inv_out == inv_in || inv_out == norm_out || !(max_norm > 0.0))
    return -2;
  hipLaunchKernelGGL(grad_clip_scale_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, part, nblk, inv_in,
                     max_norm, norm_out, inv_out);
  return MSU_CHECK_LAUNCH();
}

}  // extern "C"
