// Refine-conv weight-gradient entry points (kernels: conv3x3.h).
#include "conv3x3.h"

namespace {
// in_mode bit 1 (d2s input) and bit 0 (GELU on load) as compile-time booleans: f(d2s, gelu)
template <typename F>
int with_in_mode(int in_mode, F f) {
  switch (in_mode & 3) {
    case 0: return f(std::false_type{}, std::false_type{});
    case 1: return f(std::false_type{}, std::true_type{});
    case 2: return f(std::true_type{}, std::false_type{});
  }
  return f(std::true_type{}, std::true_type{});
}
}  // namespace

extern "C" {

long msu_conv3x3_wgrad_workspace(int nchunk, int Cin, int Cout, int dtype, int unused) {
  (void)dtype; (void)unused;
  const int CinP = (Cin + 31) / 32 * 32;
  // chunk partials [nchunk][3][Cout][3][CinP] + bias partials [nchunk][Cout] + their sum
  return (long)(nchunk + 1) * 3 * Cout * 3 * CinP + (long)nchunk * Cout;
}

// dW [Cout][Cin][3][3] f32 and db [Cout] f32 (db may be null), overwritten or (accumulate != 0)
// added to.  in_mode as in fwd.
int msu_conv3x3_wgrad2(int dtype, int in_mode, const void* X, const void* dY, float* dW, float* db,
                       float* workspace, int nchunk, int B, int H, int W, int Cin, int Cout, int accumulate,
                       void* stream) {
  if (Cout % 16 || Cin % 8 || Cout > 128 || Cin > 128 || nchunk < 1) return -2;
  const ConvGeom g = make_geom(B, H, W, Cin, Cout, msu_is16(dtype) ? 2 : 4);
  hipStream_t st = (hipStream_t)stream;
  float* part = workspace;
  float* dbpart = workspace + (long)nchunk * 3 * Cout * 3 * g.CinP;
  int rc = -3;
  int nsum = nchunk;  // partial chunks to sum
  // the widths with a persistent kernel (conv3x3_wgrad_v2_kernel); at 128 one co half per
  // workgroup, so nchunk / 2 partial chunks
  const int pw = persistent_width(msu_is16(dtype), Cin, Cout, g_conv_generic_wide != 0);
  if (pw) {
    const bf16_t* x = (const bf16_t*)X; const bf16_t* d = (const bf16_t*)dY;
    MSU_DISPATCH16(dtype, T, rc = with_in_mode(in_mode, [&](auto D2S, auto GL) {
      constexpr bool d2s = decltype(D2S)::value, gl = decltype(GL)::value;
      return pw == 96 ? launch_wgrad_v2<T, 96, d2s, gl>(g, x, d, part, dbpart, nchunk, st)
                       : launch_wgrad_v2<T, 128, d2s, gl>(g, x, d, part, dbpart, nchunk, st);
    }));
    if (rc > 0) { nsum = rc; rc = 0; }
  } else if (msu_is16(dtype)) {
    MSU_DISPATCH16(dtype, T, rc = with_in_mode(in_mode, [&](auto D2S, auto GL) {
      return wgrad_nt<T, decltype(D2S)::value, decltype(GL)::value>(g, X, dY, part, dbpart, nchunk, st);
    }));
  } else {
    rc = with_in_mode(in_mode, [&](auto D2S, auto GL) {
      return wgrad_nt<float, decltype(D2S)::value, decltype(GL)::value>(g, X, dY, part, dbpart, nchunk, st);
    });
  }
  if (rc) return rc;
  // deterministic chunk sums (one launch for the weight slab and the bias), then the
  // [dy][co][dx][ci] -> [co][ci][dy][dx] permutation
  const long slab = 3L * Cout * 3 * g.CinP;
  float* sum = dbpart + (long)nchunk * Cout;
  const ColSeg segs[2] = {{part, slab, slab, sum}, {dbpart, Cout, Cout, db}};
  // (the slab sum is workspace, always overwritten; db and the permuted dW accumulate)
  colsum_multi(segs, db ? 2 : 1, nsum, 0, st, accumulate ? 2 : 0);
  const long n = (long)Cout * Cin * 9;
  hipLaunchKernelGGL(wgrad_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sum, Cout, Cin,
                     g.CinP, dW, accumulate);
  return MSU_CHECK_LAUNCH();
}

int msu_conv3x3_wgrad(int dtype, int in_mode, const void* X, const void* dY, float* dW, float* db,
                      float* workspace, void* unused, int nchunk, int B, int H, int W, int Cin,
                      int Cout, void* stream) {
  (void)unused;
  return msu_conv3x3_wgrad2(dtype, in_mode, X, dY, dW, db, workspace, nchunk, B, H, W, Cin, Cout, 0, stream);
}

}  // extern "C"
