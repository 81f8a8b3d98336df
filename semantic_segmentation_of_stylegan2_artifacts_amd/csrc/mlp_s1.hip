// Swin MLP forward in ONE kernel with the weights streamed through LDS (torchvision MLP,
// model_parts.py:538), a template over the width C (S1W<C> below):
//
//   y = mlp.3(GELU(mlp.0(x)))      x, y: [M][C], hidden 4 C
//
// built for C = 192 (Swin-T/S stage 1, hidden 768), C = 128 (Swin-B stage 0, hidden 512) and
// C = 256 (Swin-B stage 1, hidden 1024).  The GEMM pair this replaces wrote H and GELU(H)
// (2 x 201 MB at C = 192, 8 x 128^2 tokens; 2 x 537 MB at C = 128, 8 x 256^2) and read GELU(H)
// back; here the training form writes H only (the backward's GELU' operand) and GELU(H) never
// leaves the chip.  Unlike the 96 -> 384 kernel (mlp_fused.hip) the weights (2 x 8 C^2 bytes:
// 131 / 295 / 524 KB each) do not fit one CU's LDS, so they are STREAMED.
//
// THE SLOT IMAGE.  The hidden dimension is cut into NU = 4 C / 32 chunks of 32 units.  A chunk is
// its W1 rows [32][C] and its W2 columns [C][32] (128 C bytes: 16 / 24 / 32 KB), and lies in one
// ring slot:
//   * the W1 rows PERMUTED: slot row rho holds hidden unit pi(rho), pi swapping bits 2 and 3, so
//     that fc1's accumulator registers 8s .. 8s + 7 of lane half hh hold hidden units
//     16s + 8hh .. + 7 -- consecutive, i.e. the packed GELU(H) registers are directly fc2's B
//     operand, with ONE 16-B W2 fragment read per fc2 MFMA and one 16-B H store per 8 units;
//   * W1 rows of 2 C bytes with 16-B column c at c ^ w1_swz(rho) (C = 192: (rho >> 1) & 7; C = 128
//     and 256: rho & 15), W2 rows of 64 B with column c at c ^ ((row >> 2) & 3): the 16-lane
//     groups of the ds_read_b128 fragment reads cover the 64 banks once (asserted below per width).
//
// THE RING.  Chunks go global -> LDS by LDS-DMA into a ring of NS slots (8 / 6 / 4), every wave
// of the workgroup issuing its share, and the workgroup's waves walk the chunks in step with one
// barrier per chunk.  The ring runs across the workgroup's token tiles as one flat chunk sequence
// j = 0, 1, ...: chunk j is waited for ahead of barrier j (a per-wave vmcnt count, S1Ring), may be
// read up to the end of interval j + 1 (the code between barriers j + 1 and j + 2), and interval j
// refills chunk j - 2's slot with chunk j + NS - 2.  LDS reads of the ring and of the biases are
// untracked inline asm: a compiler-visible ds_read behind a pending LDS-DMA gets a vmcnt(0) that
// drains the ring.
//
// THE PHASES (S1Wave), per 32-token wave tile:
//   * load_x: the tile's x rows stay in registers as fc1's B operand (K1 = C / 16 k steps,
//     C / 4 registers);
//   * per chunk, fc1 on MFMA (K1 MFMAs; W1 rows as A, tokens on the accumulator columns);
//   * per chunk, epi: + b1, rounded to 16 bits (stored as H), GELU, rounded again: the unfused
//     epilogues' arithmetic;
//   * per chunk, fc2 (2 NCT MFMAs) accumulates y^T over the NU chunks (NCT = C / 32 32-channel
//     tiles, C / 2 registers);
//   * y_out at a tile's last chunk: + b2, 16-B stores.
//
// WHO RUNS WHAT.  C = 128 and 192, mlp_s1_kernel: eight waves, each running every phase on a
// tile of its own (workgroup: 256 tokens).  C = 256: that register plan does not fit (x 64
// registers, y^T 128: the instantiation spills 32-48 VGPRs), so mlp_s1_kernel_pc splits the
// phases between the two waves of a SIMD: a producer runs load_x, fc1 and epi, a consumer fc2 and
// y_out, GELU(H) handed over through LDS (workgroup: 4 pairs, 128 tokens; DESIGN.md section 7,
// round 8).
#include "common.h"
#include "mfma_frag.h"

namespace {

// MSU_EXP: ablation / variant bits for timing experiments only (tools/build_exp.sh); 0 in every
// real build.  2: fragment reads one MFMA ahead instead of three; 8: no GELU (identity); 16: no H
// stores; 32: no fc2 MFMAs; 64: no fc1 MFMAs (results wrong by design for 8 / 16 / 32 / 64)
#ifndef MSU_EXP
#define MSU_EXP 0
#endif

constexpr int SW = 8;                       // waves per workgroup
constexpr int STT = 32 * SW;                // mlp_s1_kernel: tokens per workgroup tile
constexpr int PW = 4, PTT = 32 * PW;        // mlp_s1_kernel_pc: wave pairs, tokens per workgroup tile
constexpr int UH = 32;                      // hidden units per chunk (one barrier per chunk)
constexpr int FD = (MSU_EXP & 2) ? 1 : 3;   // fragment reads in flight ahead of the MFMA using one
// whether the H_OUT form issues its H stores (they count in the vmcnt waits)
template <bool H_OUT>
constexpr bool s1_h_stores = H_OUT && !(MSU_EXP & 16);

// The widths the kernel is built for: x, y [M][C], hidden 4 C.  Everything that depends on the
// width is derived here: a slot holds the chunk's W1 rows [32][C] and W2 columns [C][32]
// (128 C bytes: 16 KB at C = 128, 24 KB at 192, 32 KB at 256), both halves C / 16 1-KB DMA
// instructions.
template <int C>
struct S1W {
  static_assert(C == 128 || C == 192 || C == 256, "widths with a register plan and a conflict-free slot image");
  static constexpr int SC = C, SH = 4 * C;
  static constexpr int NU = SH / UH;          // chunks per token tile (16 / 24 / 32)
  static constexpr int K1 = C / 16;           // fc1 k steps: a lane's 16-B x loads and y stores per tile
  static constexpr int NCT = C / 32;          // 32-channel output tiles of fc2
  static constexpr int CPR = C / 8;           // 16-B columns of a W1 slot row
  // ring slots (147 KB / 128 KB).  C = 128: 6 / 7 / 8 / 9 slots measured 356 / 352-356 / 349-352 /
  // 356-359 us with H stored and 282-286 us without for all four (r07a, run-to-run spread ~3 us);
  // 8 keeps the same 96 KB in flight as the C = 192 ring.  C = 256 (mlp_s1_kernel_pc): 4 slots of
  // 32 KB, what fits beside the GELU(H) hand-over buffers
  static constexpr int NS = C == 192 ? 6 : C == 256 ? 4 : 8;
  static constexpr int W1S = UH * C;          // elements of a slot's W1 image [32][C]
  static constexpr int W2S = C * UH;          // elements of a slot's W2 image [C][32]
  static constexpr int SLOT = W1S + W2S;
  static constexpr int DMA_W1 = W1S * 2 / 1024;         // 1-KB DMA instructions of the W1 image
  static constexpr int DMA_PER_UNIT = SLOT * 2 / 1024;  // ... of a chunk (16 / 24 / 32)
  static constexpr int DMA_PER_WAVE = DMA_PER_UNIT / SW;
  static_assert(DMA_PER_WAVE * SW == DMA_PER_UNIT, "whole DMA instructions per wave");
  static_assert(NS >= 4 && (NS - 3) * DMA_PER_WAVE + 2 * (NS - 2) <= 63, "steady-state vmcnt fits the counter");
};

template <int C>
struct S1Lds {
  bf16_t ring[S1W<C>::NS * S1W<C>::SLOT];
  float b1[S1W<C>::SH];
  float b2[C];
};
// mlp_s1_kernel_pc: the same, and the GELU(H) hand-over buffers
template <int C>
struct S1PLds : S1Lds<C> {
  uint32_t hand[PW][2][2][64 * 4];  // [pair][chunk parity][k step of fc2][lane]: 16 B per lane
};
static_assert(sizeof(S1Lds<128>) <= 160 * 1024 && sizeof(S1Lds<192>) <= 160 * 1024 && sizeof(S1PLds<256>) <= 160 * 1024,
              "LDS");

struct S1Args {
  const bf16_t* x;
  const bf16_t* w1;  // [4 C][C]
  const float* b1;
  const bf16_t* w2;  // [C][4 C]
  const float* b2;
  bf16_t* y;
  bf16_t* hout;      // H_OUT: [M][4 C]
  long M;
};

// index maps: used by the kernel and by the compile-time checks of the slot image
#define S1_MAP __host__ __device__ __forceinline__ constexpr
// hidden unit (within a chunk) held by slot row rho: bits 2 and 3 swapped
S1_MAP int s1_pi(int rho) { return (rho & ~12) | ((rho & 4) << 1) | ((rho & 8) >> 1); }
// 16-B chunk swizzle of a W2 slot row (4 chunks per row)
S1_MAP int w2_swz(int row) { return (row >> 2) & 3; }
// 16-B column swizzle of W1 slot row rho.  C = 192: 384-B rows start on alternating halves of
// the 256-B bank span, so two rows share a value.  C = 128: rows are one whole bank span, every
// row starts on bank 0, and 16 rows need 16 different values; C = 256: two whole bank spans per
// row, the same (the swizzle stays inside a row's first or second 256 B).
template <int C>
S1_MAP int w1_swz(int rho) { return C == 192 ? (rho >> 1) & 7 : rho & 15; }

// ---- the slot image (byte offsets from the slot's start, a multiple of 256 B).  The fragment
// reads and the DMA below are written with these, and the asserts after them check both.
// 16-B column c of W1 slot row rho = w1_row_off(rho) + w1_col_off(c, w1_swz(rho))
template <int C>
S1_MAP uint32_t w1_row_off(int rho) { return (uint32_t)(rho * C * 2); }
S1_MAP uint32_t w1_col_off(int c, int sw) { return 16u * (uint32_t)(c ^ sw); }
// 16-B column c (0 .. 3) of W2 slot row `row` (0 .. C - 1) = w2_row_off(row) + w2_col_off(c, w2_swz(row))
template <int C>
S1_MAP uint32_t w2_row_off(int row) { return (uint32_t)(S1W<C>::W1S * 2 + row * UH * 2); }
S1_MAP uint32_t w2_col_off(int c, int sw) { return 16u * (uint32_t)(c ^ sw); }
// DMA: the W1 image's 16-B piece p (slot row p / CPR) takes this column of its weight row ...
template <int C>
S1_MAP int w1_dma_col(int p) { return (p % S1W<C>::CPR) ^ w1_swz<C>(p / S1W<C>::CPR); }
// ... and the W2 image's piece p (slot row p / 4) this 16-B column of the chunk's 32 hidden units
S1_MAP int w2_dma_col(int p) { return (p & 3) ^ w2_swz(p >> 2); }

// ds_read_b128 resolves bank conflicts within four groups of 16 lanes: lanes {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same plus 32.  Lane i (0 .. 15) of group g (0 .. 3):
constexpr int b128_group_lane(int g, int i) {
  const int l = (g & 1) == 0 ? (i < 4 ? i : i < 8 ? i + 8 : i + 12) : (i < 8 ? i + 4 : i < 12 ? i + 8 : i + 16);
  return l + 32 * (g >> 1);
}
// every fc1 / fc2 fragment read puts each group's 16 lanes on 16 distinct 16-B bank columns
template <int C>
constexpr bool s1_reads_conflict_free() {
  for (int g = 0; g < 4; ++g) {
    for (int ks = 0; ks < S1W<C>::K1; ++ks) {
      unsigned cols = 0;
      for (int i = 0; i < 16; ++i) {
        const int lane = b128_group_lane(g, i), tl = lane & 31, hh = lane >> 5;
        cols |= 1u << (((w1_row_off<C>(tl) + w1_col_off(2 * ks + hh, w1_swz<C>(tl))) >> 4) & 15);
      }
      if (cols != 0xffffu) return false;
    }
    for (int ct = 0; ct < S1W<C>::NCT; ++ct)
      for (int s = 0; s < 2; ++s) {
        unsigned cols = 0;
        for (int i = 0; i < 16; ++i) {
          const int lane = b128_group_lane(g, i), tl = lane & 31, hh = lane >> 5;
          cols |= 1u << (((w2_row_off<C>(32 * ct + tl) + w2_col_off(2 * s + hh, w2_swz(32 * ct + tl))) >> 4) & 15);
        }
        if (cols != 0xffffu) return false;
      }
  }
  return true;
}
// the DMA writes the image the reads expect: piece p lands at byte 16 p of its half of the slot
template <int C>
constexpr bool s1_dma_writes_image() {
  for (int p = 0; p < UH * S1W<C>::CPR; ++p) {
    const int rho = p / S1W<C>::CPR;
    if (w1_row_off<C>(rho) + w1_col_off(w1_dma_col<C>(p), w1_swz<C>(rho)) != 16u * (uint32_t)p) return false;
  }
  for (int p = 0; p < C * 4; ++p) {
    const int row = p >> 2;
    if (w2_row_off<C>(row) + w2_col_off(w2_dma_col(p), w2_swz(row)) != (uint32_t)(S1W<C>::W1S * 2) + 16u * (uint32_t)p)
      return false;
  }
  return true;
}
static_assert(s1_reads_conflict_free<128>() && s1_reads_conflict_free<192>() && s1_reads_conflict_free<256>(),
              "slot image: bank conflicts");
static_assert(s1_dma_writes_image<128>() && s1_dma_writes_image<192>() && s1_dma_writes_image<256>(),
              "slot image: DMA and reads disagree");

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (capped: waiting for more is always safe)
MSU_DEV void wait_vmcnt_le(int n) {
  switch (n < 0 ? 0 : (n > 40 ? 40 : n)) {
#define MSU_W(k) case k: wait_vmcnt<k>(); break;
    MSU_W(0) MSU_W(1) MSU_W(2) MSU_W(3) MSU_W(4) MSU_W(5) MSU_W(6) MSU_W(7) MSU_W(8) MSU_W(9)
    MSU_W(10) MSU_W(11) MSU_W(12) MSU_W(13) MSU_W(14) MSU_W(15) MSU_W(16) MSU_W(17) MSU_W(18) MSU_W(19)
    MSU_W(20) MSU_W(21) MSU_W(22) MSU_W(23) MSU_W(24) MSU_W(25) MSU_W(26) MSU_W(27) MSU_W(28) MSU_W(29)
    MSU_W(30) MSU_W(31) MSU_W(32) MSU_W(33) MSU_W(34) MSU_W(35) MSU_W(36) MSU_W(37) MSU_W(38) MSU_W(39)
    MSU_W(40)
#undef MSU_W
    default: wait_vmcnt<0>();
  }
}

template <int OFF>
MSU_DEV bf16x8 ds_b128_untracked(uint32_t addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}

// the ring's barrier: LDS-DMA stays in flight across it (no __syncthreads: its fence drains vmcnt)
MSU_DEV void s1_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// chunk q (0 .. NU - 1) of the weights into ring slot `slot`: wave `wave`'s share (C / 64) of the
// chunk's C / 8 1-KB DMA instructions (W1 rows permuted by pi and chunk-swizzled; W2 columns
// chunk-swizzled), every wave of the workgroup alike
template <int C>
MSU_DEV void s1_dma_unit(const S1Args& A, bf16_t* ring, int wave, int lane, int q, int slot) {
  using W = S1W<C>;
  bf16_t* base = ring + slot * W::SLOT;
  const int ln = opaque(lane);
#pragma unroll
  for (int r = 0; r < W::DMA_PER_WAVE; ++r) {
    const int i = wave + SW * r;  // instruction (wave-uniform)
    if (i < W::DMA_W1) {
      const int p = 64 * i + ln, rho = p / W::CPR;
      glds16(A.w1 + (long)(UH * q + s1_pi(rho)) * W::SC + 8 * w1_dma_col<C>(p), base + 512 * i);
    } else {
      const int i2 = i - W::DMA_W1;
      const int p = 64 * i2 + ln, row = p >> 2;
      glds16(A.w2 + (long)row * W::SH + UH * q + 8 * w2_dma_col(p), base + W::W1S + 512 * i2);
    }
  }
}

// ---- the ring's bookkeeping, one per wave.  `issued`: the vector-memory ops this wave has issued
// (wave-uniform): its DMA share of every chunk, its x loads (K1 per tile), H stores (2 per chunk)
// and y stores (2 NCT per tile), whichever of them its role has.  mark[]: the count right after
// each pending chunk's DMA (a queue of NS - 2, the chunk waited for next first), so that a wait
// lets every younger op stay in flight.  Stores are counted only when the whole wave issues them
// (full tile rows): an uncounted op only makes a wait stricter.
template <int C>
struct S1Ring {
  using W = S1W<C>;
  static constexpr int NS = W::NS, NU = W::NU, DPW = W::DMA_PER_WAVE;
  // the ops younger than chunk j's DMA in steady state (full tiles, no tile boundary among them):
  // the DMA of chunks j + 1 .. j + NS - 3 and, for a wave that stores H, the stores of intervals
  // j - NS + 2 .. j - 1
  static constexpr int steady(bool h_stores) { return (NS - 3) * DPW + (h_stores ? 2 * (NS - 2) : 0); }

  const S1Args& A;
  bf16_t* const ring;
  const int wave, lane;
  const long nunits;  // chunks this workgroup walks: (its tiles) x NU
  int issued = 0;
  int mark_x = 0;     // the count right after the x loads of the tile in registers
  int mark[NS - 2];
  int qn = (NS - 2) % NU, sn = NS - 2;  // the next chunk to issue (weights chunk, ring slot)

  MSU_DEV S1Ring(const S1Args& a, bf16_t* r, int w, int l, long n) : A(a), ring(r), wave(w), lane(l), nunits(n) {}

  // the first NS - 2 chunks, before the first barrier of the loop
  MSU_DEV void prologue() {
#pragma unroll
    for (int s = 0; s < NS - 2; ++s) {
      if (s < nunits) {
        s1_dma_unit<C>(A, ring, wave, lane, s % NU, s);
        issued += DPW;
      }
      mark[s] = issued;
    }
  }
  // ahead of barrier j (j < nunits): this wave's share of chunk j's DMA has landed
  template <int STEADY>
  MSU_DEV void wait_chunk() {
    const int younger = issued - mark[0];
    if (younger >= STEADY) wait_vmcnt<STEADY>();
    else wait_vmcnt_le(younger);
  }
  // behind barrier j: every wave is done with chunk j - 2's slot; chunk j + NS - 2 goes there.
  // Once per interval, whether or not a chunk is left to issue
  MSU_DEV void refill(long j) {
#pragma unroll
    for (int s = 0; s < NS - 3; ++s) mark[s] = mark[s + 1];
    if (j + NS - 2 < nunits) {
      s1_dma_unit<C>(A, ring, wave, lane, qn, sn);
      issued += DPW;
    }
    mark[NS - 3] = issued;
    qn = qn + 1 == NU ? 0 : qn + 1;
    sn = sn + 1 == NS ? 0 : sn + 1;
  }
  MSU_DEV void count_x() {
    issued += W::K1;
    mark_x = issued;
  }
  MSU_DEV void wait_x() { wait_vmcnt_le(issued - mark_x); }
  MSU_DEV void count_stores(int n) { issued += n; }
};

// the biases into LDS, before any LDS-DMA is in flight (this barrier drains nothing)
template <int C>
MSU_DEV void s1_stage_biases(const S1Args& A, S1Lds<C>& L, int tid) {
  for (int s = tid; s < S1W<C>::SH; s += 64 * SW) L.b1[s] = A.b1[s];
  for (int s = tid; s < C; s += 64 * SW) L.b2[s] = A.b2[s];
  __syncthreads();
}

// ---- the phases, for the wave whose 32-token tile starts at row `row0` (workgroup tile t:
// t * TT + 32 * the wave's place in it).  Lane (tl, hh) = (lane & 31, lane >> 5) works on token
// row0 + tl; the register arrays are the caller's.
template <typename T, int C>
struct S1Wave {
  using W = S1W<C>;
  static constexpr int SC = W::SC, SH = W::SH, NU = W::NU, K1 = W::K1, NCT = W::NCT, SLOT = W::SLOT;
  const S1Args& A;
  S1Ring<C>& ring;
  const int tl, hh;
  // untracked-read lane addresses (bytes)
  const uint32_t ring0;
  const uint32_t a1_lane;  // + slot, + 16 * pos(ks)
  const int w1sw;
  const uint32_t a2_lane;  // + slot, + 2048 ct, + 16 * pos
  const int w2sw;          // (32 ct + tl: same swizzle)
  const uint32_t b1_lane, b2_lane;

  MSU_DEV S1Wave(const S1Args& a, S1Lds<C>& L, S1Ring<C>& r, int lane)
      : A(a), ring(r), tl(lane & 31), hh(lane >> 5), ring0(lds_u32(L.ring)), a1_lane(w1_row_off<C>(tl)),
        w1sw(w1_swz<C>(tl)), a2_lane(w2_row_off<C>(tl)), w2sw(w2_swz(tl)),
        b1_lane(lds_u32(L.b1) + 4u * (uint32_t)(8 * hh)), b2_lane(lds_u32(L.b2) + 4u * (uint32_t)(4 * hh)) {}

  // the tile's token rows as fc1's B operand: lane (token tl, half hh) holds k = 16 ks + 8 hh .. + 7
  MSU_DEV void load_x(long row0, u32x4 (&xc)[K1]) {
    const long row = row0 + tl;
    const bool ok = row < A.M;
    const bf16_t* p = A.x + (ok ? row : 0) * SC + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < K1; ++ks) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * ks);
      xc[ks] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
    ring.count_x();
  }

  // h = W1[chunk in `slot`] . x^T
  MSU_DEV void fc1(int slot, const u32x4 (&xc)[K1], f32x16& h) {
    const uint32_t a1 = ring0 + (uint32_t)(slot * SLOT * 2) + a1_lane;
    h = f32x16{0};
    bf16x8 wf[FD + 1];
    auto addr1 = [&](int ks) { return a1 + w1_col_off(2 * ks + hh, w1sw); };
    unroll_for<FD>([&](auto KS) { wf[decltype(KS)::value] = ds_b128_untracked<0>(addr1(decltype(KS)::value)); });
    unroll_for<K1>([&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      if constexpr (ks + FD < K1) wf[(ks + FD) % (FD + 1)] = ds_b128_untracked<0>(addr1(ks + FD));
      lds_wait_tie<(ks + FD < K1 ? FD : K1 - 1 - ks)>(wf[ks % (FD + 1)]);
      if constexpr (MSU_EXP & 64) {
        const bf16x8 wv = wf[ks % (FD + 1)];
        const u32x4 xv = xc[ks];
        asm volatile("" ::"v"(wv), "v"(xv));
      } else h = Fmt16<T>::mma32(wf[ks % (FD + 1)], __builtin_bit_cast(bf16x8, xc[ks]), h);
    });
  }
  // fc1 of chunk q of a tile: its first chunk waits for the tile's x rows, and xc is free for the
  // next tile's (from row `next0`, if there is one: `more`) once its last fc1 has issued
  MSU_DEV void fc1_step(int q, int slot, bool more, long next0, u32x4 (&xc)[K1], f32x16& h) {
    if (q == 0) ring.wait_x();
    fc1(slot, xc, h);
    if (q == NU - 1 && more) load_x(next0, xc);
  }

  // + b1, 16-bit H (stored), GELU, 16-bit GELU(H): registers 8s + e <-> hidden 32 q + 16 s + 8 hh + e
  template <bool H_OUT>
  MSU_DEV void epi(int q, long row0, const f32x16& h, u32x4 (&g)[2]) {
    u32x4 bq[4];
    unroll_for<4>([&](auto BI) {
      constexpr int bi = decltype(BI)::value;
      bq[bi] = __builtin_bit_cast(u32x4, ds_b128_untracked<(bi >> 1) * 64 + (bi & 1) * 16>(
                                             b1_lane + 4u * (uint32_t)(UH * q)));
    });
    lds_wait_tie<0>(bq[0], bq[1], bq[2], bq[3]);
    const long hrow = row0 + tl;
    const bool hok = hrow < A.M;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float uu[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uu[e] = round16<T>(h[8 * s + e] + __uint_as_float(bq[2 * s][e]));
        uu[4 + e] = round16<T>(h[8 * s + 4 + e] + __uint_as_float(bq[2 * s + 1][e]));
      }
      if constexpr (H_OUT) {
        const u32x4 hv = {pack2<T>(uu[0], uu[1]), pack2<T>(uu[2], uu[3]), pack2<T>(uu[4], uu[5]),
                          pack2<T>(uu[6], uu[7])};
        if constexpr (MSU_EXP & 16) {
          const u32x4 hv2 = hv;
          asm volatile("" ::"v"(hv2));
        }
        else if (hok) *reinterpret_cast<u32x4*>(A.hout + hrow * SH + UH * q + 16 * s + 8 * hh) = hv;
      }
      uint32_t gp[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x2 gv = (MSU_EXP & 8) ? f32x2{uu[2 * e], uu[2 * e + 1]}
                                       : gelu_fast2(f32x2{uu[2 * e], uu[2 * e + 1]});  // bitwise two gelu_fast
        gp[e] = pack2<T>(gv.x, gv.y);
      }
      g[s] = u32x4{gp[0], gp[1], gp[2], gp[3]};
    }
    if (s1_h_stores<H_OUT> && row0 + 32 <= A.M) ring.count_stores(2);
  }

  // y^T[c][t] += W2[c][chunk in `slot`] . GELU(H)^T: C / 32 32-channel tiles, two 16-deep k steps.
  // G_PENDING: g[0], g[1] are untracked LDS reads the caller has just issued (ahead of every read
  // here); the first fragment's wait covers them
  template <bool G_PENDING>
  MSU_DEV void fc2(int slot, u32x4 (&g)[2], f32x16 (&yacc)[NCT]) {
    const uint32_t a2 = ring0 + (uint32_t)(slot * SLOT * 2) + a2_lane;
    auto addr2 = [&](int ct, int s) { return a2 + (uint32_t)(ct * 32 * UH * 2) + w2_col_off(2 * s + hh, w2sw); };
    bf16x8 af[FD + 1];
    unroll_for<FD>([&](auto I) {
      constexpr int i = decltype(I)::value;
      af[i] = ds_b128_untracked<0>(addr2(i % NCT, i / NCT));
    });
    unroll_for<2 * NCT>([&](auto I) {
      constexpr int i = decltype(I)::value, s = i / NCT, ct = i % NCT;
      if constexpr (i + FD < 2 * NCT) af[(i + FD) % (FD + 1)] = ds_b128_untracked<0>(addr2((i + FD) % NCT, (i + FD) / NCT));
      constexpr int behind = i + FD < 2 * NCT ? FD : 2 * NCT - 1 - i;  // reads issued after fragment i's
      if constexpr (G_PENDING && i == 0) lds_wait_tie<behind>(af[0], g[0], g[1]);
      else lds_wait_tie<behind>(af[i % (FD + 1)]);
      if constexpr (MSU_EXP & 32) {
        const bf16x8 av = af[i % (FD + 1)];
        const u32x4 gv = g[s];
        asm volatile("" ::"v"(av), "v"(gv));
      } else yacc[ct] = Fmt16<T>::mma32(af[i % (FD + 1)], __builtin_bit_cast(bf16x8, g[s]), yacc[ct]);
    });
  }

  // tile epilogue: y = y^T + b2, and y^T = 0 for the next tile; lane (token tl) holds channels
  // 32 ct + 8 r4 + 4 hh + i in register 4 r4 + i; a permlane32 swap pairs the halves into 8
  // consecutive channels per lane
  MSU_DEV void y_out(long row0, f32x16 (&yacc)[NCT]) {
    const long row = row0 + tl;
    const bool ok = row < A.M;
    bf16_t* yr = A.y + (ok ? row : 0) * SC;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      uint32_t w[8];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        u32x4 bq;
        asm volatile("ds_read_b128 %0, %1" : "=v"(bq) : "v"(b2_lane + 4u * (uint32_t)(ct * 32 + 8 * r4)));
        lds_wait_tie<0>(bq);
        w[2 * r4] = pack2<T>(yacc[ct][4 * r4] + __uint_as_float(bq[0]), yacc[ct][4 * r4 + 1] + __uint_as_float(bq[1]));
        w[2 * r4 + 1] = pack2<T>(yacc[ct][4 * r4 + 2] + __uint_as_float(bq[2]),
                                 yacc[ct][4 * r4 + 3] + __uint_as_float(bq[3]));
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const auto s0 = __builtin_amdgcn_permlane32_swap(w[4 * p], w[4 * p + 2], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(w[4 * p + 1], w[4 * p + 3], false, false);
        const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
        if (ok) *reinterpret_cast<u32x4*>(yr + ct * 32 + 16 * p + 8 * hh) = v;
      }
      yacc[ct] = f32x16{0};
    }
    if (row0 + 32 <= A.M) ring.count_stores(2 * NCT);
  }
};

// ---------------------------------------------------------------- C = 128, 192: one role
// Every wave runs every phase on a 32-token tile of its own: in interval j (the code behind
// barrier j) fc1, epi and fc2 of chunk j, and y_out at a tile's last chunk.  A workgroup walks
// the tiles first, first + G, ...; every wave of it executes 1 + nunits barriers, nunits from
// blockIdx, gridDim and M alone (the only return is ahead of all of them and uniform over the
// workgroup; rows past M only mask loads and stores).
template <typename T, bool H_OUT, int C>
__global__ void __launch_bounds__(64 * SW) mlp_s1_kernel(S1Args A) {
  using W = S1W<C>;
  using R = S1Ring<C>;
  constexpr int NU = W::NU, NS = W::NS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  S1Lds<C>& L = *reinterpret_cast<S1Lds<C>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long ntiles = (A.M + STT - 1) / STT;
  const int G = gridDim.x;
  const long first = blockIdx.x;
  if (first >= ntiles) return;
  const long mine = (ntiles - 1 - first) / G + 1;
  const long nunits = mine * NU;
  s1_stage_biases<C>(A, L, tid);

  R ring(A, L.ring, wave, lane, nunits);
  S1Wave<T, C> w(A, L, ring, lane);
  auto row0 = [&](long t) { return t * STT + 32 * wave; };
  u32x4 xc[W::K1];
  f32x16 h, yacc[W::NCT];
#pragma unroll
  for (int ct = 0; ct < W::NCT; ++ct) yacc[ct] = f32x16{0};
  w.load_x(row0(first), xc);
  ring.prologue();

  // interval j: chunk j = weights chunk q in ring slot `slot` of tile `tile`
  int q = 0, slot = 0;
  long tile = first;
  for (long j = 0; j < nunits; ++j) {
    ring.template wait_chunk<R::steady(s1_h_stores<H_OUT>)>();
    s1_barrier();  // chunk j's DMA (every wave's share) has landed
    ring.refill(j);
    w.fc1_step(q, slot, tile + G < ntiles, row0(tile + G), xc, h);
    u32x4 g[2];
    w.template epi<H_OUT>(q, row0(tile), h, g);
    w.template fc2<false>(slot, g, yacc);
    if (q == NU - 1) {
      w.y_out(row0(tile), yacc);
      tile += G;
    }
    q = q + 1 == NU ? 0 : q + 1;
    slot = slot + 1 == NS ? 0 : slot + 1;
  }
  wait_vmcnt<0>();  // no LDS-DMA outstanding when the workgroup retires
}

// ---------------------------------------------------------------- C = 256: producer / consumer
// The same phases, ring and slot image with the work of a 32-token tile split between the two
// waves of a SIMD (waves p and p + 4, p = 0 .. 3; workgroup tile: 4 pairs, 128 tokens):
//   * the PRODUCER (wave p) holds x (C / 4 = 64 registers) and the fc1 accumulator; per chunk it
//     runs fc1 and epi and writes the packed GELU(H) -- fc2's B operand, 2 x 16 B per lane --
//     into the pair's hand-over buffer;
//   * the CONSUMER (wave p + 4) holds y^T (C / 2 = 128 registers); per chunk it reads those 32 B
//     back into the same lanes, runs fc2 against the chunk's W2 columns, and y_out per tile.
// The older half of the workgroup has the VALU-heavy role.  Both roles issue their wave's share
// of every chunk's DMA (4 of its 32 instructions) and keep a ring count of their own.  The
// hand-over is double-buffered by chunk parity and ordered by the ring's one barrier per chunk:
// in interval j (the code between barrier j and barrier j + 1) the producer works on chunk j
// (slot j's W1 rows, buffer j & 1) and the consumer on chunk j - 1 (slot j - 1's W2 columns,
// buffer (j - 1) & 1):
//   * the producer's ds_writes of chunk j are waited for (lgkmcnt(0), same asm statement) before
//     it arrives at barrier j + 1, which releases the consumer's reads of them;
//   * the consumer's reads of buffer j & 1 (interval j + 1) have returned (fc2's first
//     lds_wait_tie, ahead of the MFMAs that use them) before it arrives at barrier j + 2, behind
//     which the producer overwrites that buffer with chunk j + 2;
//   * chunk j - 1's slot is read up to the end of interval j, which is why interval j refills
//     chunk j - 2's slot and no younger one.
// BARRIERS: every wave of a workgroup executes 1 + (nunits + 1) of them, nunits = mine * NU from
// blockIdx, gridDim and M alone: the __syncthreads of s1_stage_biases and the s1_barrier of each
// j = 0 .. nunits in whichever role loop the wave runs (both loops have the same bounds, and the
// barrier and the refill behind it stand outside the `cur` / `j > 0` guards, so each role calls
// refill once per interval); the only return is ahead of all of them and is uniform over the
// workgroup, and rows past M only mask loads and stores.  By hand, 256 CUs, NU = 32:
// M = 1: ntiles = 1, one workgroup, mine = 1, nunits = 32: 1 + 33 in all 8 waves (pairs 1-3
// work on zero rows); M = 129: ntiles = 2, two workgroups with mine = 1: 1 + 33 each;
// M = 128 * 257 + 5: ntiles = 258 on 256 workgroups, mine = (257 - first) / 256 + 1 = 2 for
// workgroups 0 and 1 (nunits = 64: 1 + 65) and 1 for the others (1 + 33).
template <typename T, bool H_OUT, int C>
__global__ void __launch_bounds__(64 * SW) mlp_s1_kernel_pc(S1Args A) {
  using W = S1W<C>;
  using R = S1Ring<C>;
  constexpr int NU = W::NU, NS = W::NS, K1 = W::K1, NCT = W::NCT, DPW = W::DMA_PER_WAVE;
  static_assert(SW == 2 * PW, "a producer and a consumer per SIMD");
  // outstanding at most K1 + (NS - 2) DPW + 2 (NS - 1) (producer, across a tile boundary) and
  // 2 NCT + (NS - 2) DPW (consumer)
  static_assert(K1 + (NS - 2) * DPW + 2 * (NS - 1) <= 63 && 2 * NCT + (NS - 2) * DPW <= 63, "vmcnt fits the counter");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  S1PLds<C>& L = *reinterpret_cast<S1PLds<C>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = wave & (PW - 1);
  const bool producer = wave < PW;  // wave-uniform
  const long ntiles = (A.M + PTT - 1) / PTT;
  const int G = gridDim.x;
  const long first = blockIdx.x;
  if (first >= ntiles) return;  // uniform over the workgroup, ahead of every barrier
  const long mine = (ntiles - 1 - first) / G + 1;
  const long nunits = mine * NU;  // both role loops run j = 0 .. nunits: one barrier each
  s1_stage_biases<C>(A, L, tid);

  R ring(A, L.ring, wave, lane, nunits);
  S1Wave<T, C> w(A, L, ring, lane);
  auto row0 = [&](long t) { return t * PTT + 32 * pair; };
  const uint32_t hand_lane = lds_u32(&L.hand[pair][0][0][0]) + 16u * (uint32_t)lane;  // + 2048 parity, + 1024 s

  if (producer) {
    u32x4 xc[K1];
    f32x16 h;
    w.load_x(row0(first), xc);
    ring.prologue();
    int q = 0, slot = 0;
    long tile = first;
    for (long j = 0; j <= nunits; ++j) {
      const bool cur = j < nunits;
      if (cur) ring.template wait_chunk<R::steady(s1_h_stores<H_OUT>)>();
      // chunk j's DMA (every wave's share) has landed; the consumers are done with chunk j - 2's
      // slot and hand-over buffer
      s1_barrier();
      ring.refill(j);
      if (cur) {
        w.fc1_step(q, slot, tile + G < ntiles, row0(tile + G), xc, h);
        u32x4 g[2];
        w.template epi<H_OUT>(q, row0(tile), h, g);
        // the hand-over, complete before this wave arrives at the next barrier
        asm volatile("ds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     :: "v"(hand_lane + 2048u * (uint32_t)(j & 1)), "v"(g[0]), "v"(g[1]) : "memory");
        if (q == NU - 1) tile += G;
        q = q + 1 == NU ? 0 : q + 1;
        slot = slot + 1 == NS ? 0 : slot + 1;
      }
    }
  } else {
    ring.prologue();
    f32x16 yacc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) yacc[ct] = f32x16{0};
    int qp = 0, slotp = 0;  // chunk j - 1: the one this role works on in interval j
    long tilep = first;
    for (long j = 0; j <= nunits; ++j) {
      if (j < nunits) ring.template wait_chunk<R::steady(false)>();
      // chunk j's DMA has landed; the producers' hand-over of chunk j - 1 is complete
      s1_barrier();
      ring.refill(j);
      if (j > 0) {
        // the two hand-over reads go first; fc2's first fragment wait covers them
        const uint32_t hb = hand_lane + 2048u * (uint32_t)((j - 1) & 1);
        u32x4 g[2];
        g[0] = __builtin_bit_cast(u32x4, ds_b128_untracked<0>(hb));
        g[1] = __builtin_bit_cast(u32x4, ds_b128_untracked<1024>(hb));
        w.template fc2<true>(slotp, g, yacc);
        if (qp == NU - 1) {
          w.y_out(row0(tilep), yacc);
          tilep += G;
        }
        qp = qp + 1 == NU ? 0 : qp + 1;
        slotp = slotp + 1 == NS ? 0 : slotp + 1;
      }
    }
  }
  wait_vmcnt<0>();  // no LDS-DMA outstanding when the workgroup retires
}

// C = 256 takes the producer / consumer kernel (128-token workgroup tiles), the other widths the
// one-role kernel (256-token tiles)
template <typename T, bool H_OUT, int C>
int launch_s1(const S1Args& a, hipStream_t st) {
  constexpr bool PC = C == 256;
  constexpr int TT = PC ? PTT : STT;
  constexpr size_t LDS = PC ? sizeof(S1PLds<C>) : sizeof(S1Lds<C>);
  void (*kern)(S1Args);
  if constexpr (PC) kern = mlp_s1_kernel_pc<T, H_OUT, C>;
  else kern = mlp_s1_kernel<T, H_OUT, C>;
  static bool attr_set = false;  // one per instantiation: each kernel needs its own attribute
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS) != hipSuccess)
      return -4;
    attr_set = true;
  }
  const long ntiles = (a.M + TT - 1) / TT;
  long grid = msu_num_cus();
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * SW), LDS, st, a);
  return MSU_CHECK_LAUNCH();
}

}  // namespace

// whether the streamed-weight kernel is built for x, y [M][C] (hidden 4 C)
int msu_mlp_s1_width(int C) { return C == 128 || C == 192 || C == 256; }

// the streamed-weight form of msu_mlp_fused_fwd (mlp_fused.hip dispatches here for the widths of
// msu_mlp_s1_width: Swin-B stage 0, C = 128, Swin-T/S stage 1, C = 192, and Swin-B stage 1, C = 256)
int msu_mlp_s1_launch(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                      void* y, void* h, long M, int C, void* stream) {
  S1Args a{};
  a.x = (const bf16_t*)x;
  a.w1 = (const bf16_t*)w1;
  a.b1 = b1;
  a.w2 = (const bf16_t*)w2;
  a.b2 = b2;
  a.y = (bf16_t*)y;
  a.hout = (bf16_t*)h;
  a.M = M;
  hipStream_t st = (hipStream_t)stream;
#define MSU_S1_WIDTH(CC)                                                \
  if (C == CC) {                                                        \
    if (h != nullptr) {                                                 \
      MSU_DISPATCH16(dtype, T, return (launch_s1<T, true, CC>(a, st))); \
    } else {                                                            \
      MSU_DISPATCH16(dtype, T, return (launch_s1<T, false, CC>(a, st)));\
    }                                                                   \
    return -3;                                                          \
  }
  MSU_S1_WIDTH(128)
  MSU_S1_WIDTH(192)
  MSU_S1_WIDTH(256)
#undef MSU_S1_WIDTH
  return -2;
}
