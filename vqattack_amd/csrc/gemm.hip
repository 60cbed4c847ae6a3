// fp32 GEMM of the frozen encoders' projections on the bf16 matrix pipe (gfx950 / MI355X):  C = A . B (+ bias)  with A
// fp32 [M, K] (row stride lda), B a frozen weight pre-packed into three bf16 planes, C fp32 [M, N] (row stride ldc).
//
// Why: gfx950 has no xf32 MFMA and its f32-input MFMA runs at 1/16 of the bf16 rate.  An fp32 value splits exactly into
// three bf16 pieces  a = a0 + a1 + a2  (a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1), both subtractions exact
// in fp32), and the six products that carry fp32's precision -- a0b0, a0b1, a1b0, a0b2, a1b1, a2b0 ("bf16x6") -- cost
// 6/16 of one fp32 MFMA.  The dropped terms a1b2 + a2b1 + a2b2 are <= ~2^-26 |ab| together, below the half-ulp fp32
// rounds every product to.  Non-finite a (or an a0 that rounds to inf): a1 = a2 = 0, so inf / NaN propagate as in fp32.
//
// B (the weight) is split ONCE by vqa_gemm_pack_b into the kernel's fragment order; only A is split on the fly, once per
// workgroup and k-step, into three LDS planes that every wave then reads as MFMA fragments.
//
// Tile: 256 x 128 outputs per workgroup of 8 waves (4 along M x 2 along N, 64 x 64 each = 4 x 4 tiles of
// v_mfma_f32_16x16x32_bf16), BK = 32.  LDS per k-step: A 16 m-tiles x 3 planes x 1 KiB + B 8 n-tiles x 3 planes x 1 KiB
// = 72 KiB, double-buffered = 144 KiB (one workgroup per CU, 2 waves per SIMD).  Every LDS image is "fragment order":
// 1 KiB per (tile, plane), lane l's 16 bytes at l * 16, so every ds_read_b128 / ds_write_b128 of a wave is one linear,
// conflict-free KiB.  Per k-step a wave issues 24 fragment reads and 96 MFMAs.  The k-loop is: issue the global loads of
// step k+1 (A into registers, B straight into the other LDS buffer), run the MFMAs of step k, split + write A of step
// k+1 into the other buffer, wait for the B loads, one barrier.
//
// Staging of B: vqa_gemm_pack_b wrote B in fragment order, so the LDS image of a k-step is a plain copy of its run of
// packed B, and thread tid's 16-byte piece p goes to (p * 512 + tid) * 16 = a wave-uniform base + lane * 16.  That is
// the form a direct-to-LDS load writes (stage_b16: global_load_lds_dwordx4), so the 256 x 128 and 128 x 256 kernels
// and their _epi copies move B without a register or a ds_write (3 / 6 pieces per thread and k-step; measured
// 1.03-1.09x per kernel over staging through registers, profiles/r12/README.md).  Such a load is a pending LDS write
// on the vector-memory counter: every wave waits for its own (stage_b_wait) ahead of the barrier that ends the step,
// and the buffer it targets was last read before the barrier that began the step.  All LDS is ONE __shared__ array.
// gemm_bf16x6_small_kernel keeps the register staging (rb[]): it is what the tests compare the bits against.
//
// Packed B ("vqa_gemm_pack_b"): bf16 [K/32][N/16][3 planes][64 lanes][8]; element (k, n) sits in plane tile
// (k / 32, n / 16) at lane (n % 16) + 16 * ((k % 32) / 8), slot k % 8 -- the B-operand map of the 16x16x32 MFMA.  The
// 8 n-tiles x 3 planes a workgroup stages per k-step are therefore one contiguous 24 KiB run.
//
// Epilogue of the large tiles: the A and B operand maps of the 16x16x32 MFMA are the same map (row or column on
// lane & 15, k-chunk on lane >> 4), so the eight large-tile kernels hand the instruction (B fragment, A fragment) and get
// the transposed tile: a lane's four accumulator registers are four consecutive COLUMNS of one row.  Each of a lane's 16
// tiles is then one 16-byte store (and, in the GELU' kernel, one 16-byte load of h) instead of four dword accesses that
// each cover 4 rows x 64 bytes, and a row's four tiles are issued back to back (whole 128-byte lines); the same products are summed in the same order per element, so the bits are those of
// gemm_bf16x6_small_kernel, which keeps the instruction's own order and dword stores.  The 16-byte form needs C, bias
// and aux on 16-byte boundaries and ldc, ldaux % 4 == 0 (GemmArgs::vec, worked out by the wrappers); the entry points
// still take 4-byte-aligned pointers and any stride >= N, which run the same lane map with dword accesses.
//
// Rounds: at 144 KiB of LDS the large tiles run one workgroup per CU, so a launch takes ceil(tiles / CUs) rounds of equal
// length and a last round that is a quarter full costs a whole one.  gemm_bf16x6_half_kernel (128 x 128, 96 KiB, the
// same loop with half the MFMAs per k-step, the same bits) takes the rows behind the last full round where they fit
// one round of half tiles: vqa_gemm_bf16x6_tail launches the two back to back, cut at the row ops.gemm_tail_plan names.
//
// Groups: gemm_bf16x6_grouped_kernel<EPI> runs the 128 x 256 tiles of up to four products with one (N, K) -- the expert
// FFNs of a multiway block -- as one grid, so a product too small for a launch of its own fills the last round of a
// large one (vqa_gemm_bf16x6_grouped; the groups travel in the kernel arguments).  The same loop, the same bits per group.
//
// Persistent: gemm_bf16x6_persistent_kernel runs the 128 x 256 tiles of one product as ONE launch of one workgroup per
// CU, each walking a fixed, blockIdx-derived list of tiles (vqa_gemm_bf16x6_persistent).  The last k-step of a tile
// stages the first k-step of the workgroup's next tile in place of the wide kernel's redundant reload, so only a
// workgroup's first tile waits for its operands with the matrix pipe idle.  The same loop, the same bits.
//
// Deterministic: fixed summation order (per k-step the products a2b0, a1b1, a0b2, a1b0, a0b1, a0b0 in turn, k-steps in
// order), no split-K, no atomics.  Rows >= M are read clamped to row M-1 and never stored.
#include "common.hpp"
#include "gelu.hpp"

namespace vqa {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGemmBM = 256, kGemmBN = 128, kGemmBK = 32;
constexpr int kGemmThreads = 512;
constexpr int kGemmMT = kGemmBM / 16, kGemmNT = kGemmBN / 16;        // 16 m-tiles, 8 n-tiles per workgroup
constexpr int kTileBytes = 64 * 16;                                    // one (tile, plane) fragment image: 1 KiB
constexpr int kGemmABytes = kGemmMT * 3 * kTileBytes;                  // 48 KiB
constexpr int kGemmBBytes = kGemmNT * 3 * kTileBytes;                  // 24 KiB
constexpr int kGemmStage = kGemmABytes + kGemmBBytes;                  // 72 KiB
constexpr int kGemmBPieces = kGemmBBytes / 16 / kGemmThreads;          // 3 x 16 B of B per thread and k-step
constexpr int kWideLoadPair = 12;                                      // MFMAs behind each pair of global loads of the next step

// split2 / split8 (a -> its three bf16 planes) live in common.hpp: the attention forward splits with the same body.

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4): the wave's 64 pieces land at
// lds + lane * 16, lds wave-uniform.  A pending LDS write on the vector-memory counter until stage_b_wait().
__device__ __forceinline__ void stage_b16(const bf16x8* src, char* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,   // address-space casts are C casts
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
// Every vector-memory operation of this wave has completed (s_waitcnt vmcnt(0)): ahead of the barrier behind which the
// other waves read what stage_b16 wrote.
__device__ __forceinline__ void stage_b_wait() { __builtin_amdgcn_s_waitcnt(0x0f70); }

struct GemmArgs {
  const float* A;
  const bf16x8* B;     // packed planes
  const float* bias;   // nullable
  float* C;
  long lda, ldc, M;
  int N, K;
  int vec;             // large-tile kernels: C, bias (and aux) are 16-byte aligned and ldc (ldaux) % 4 == 0 (gemm_vec_ok)
};

// Four consecutive floats of a row: one 16-byte access where the wrapper found everything aligned (VEC), four dwords
// where it did not.
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p) {
  if constexpr (VEC) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, const f32x4& v) {
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
  }
}

// Plain epilogue of a wave's 64 x 64 block at (row0, col0).  The large-tile kernels pass the MFMA its operands in the
// order (B fragment, A fragment), so an accumulator tile is the transpose of the instruction's own layout: register r
// of tile (i, j) is row i * 16 + (lane & 15), column j * 16 + (lane >> 4) * 4 + r -- four consecutive columns, one
// 16-byte store per tile (16 per lane) instead of four dword stores down a column.  Same products in the same order
// per element: the bits do not change.  Fully unrolled, rows >= M are not stored.  Order: i outer, j inner, see
// gemm_epilogue_rows.
template <bool VEC, bool FULL>
__device__ __forceinline__ void gemm_store_rows(const f32x4 (&acc)[4][4], const GemmArgs& g, long row0, int col0, int lane) {
  const int colq = col0 + (lane >> 4) * 4;
  // the bias is added to all 16 tiles ahead of the first store: the memory counter is one for loads and stores, in order,
  // so a bias load consumed behind a store (or behind a row guard, where the compiler no longer knows what is
  // outstanding) waits for that store to be acknowledged
  f32x4 v[4][4];
  if (g.bias) {
    f32x4 bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = load4<VEC>(g.bias + colq + j * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j] + bv[j];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j];
  }
  // a row's four tiles back to back: its 256 bytes -- two whole 128-byte lines -- leave in consecutive stores
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = row0 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (FULL || row < g.M) store4<VEC>(g.C + row * g.ldc + colq + j * 16, v[i][j]);
  }
}

// FULL: all 64 rows of the wave's block are below M (row0 is the wave's: uniform), so nothing is guarded and the 16
// stores are one basic block.  The scalar path (a misaligned pointer or an odd stride) has the guarded form only.
__device__ __forceinline__ void gemm_store(const f32x4 (&acc)[4][4], const GemmArgs& g, long row0, int col0, int lane) {
  if (!g.vec) {
    gemm_store_rows<false, false>(acc, g, row0, col0, lane);
  } else if (__builtin_amdgcn_readfirstlane(row0 + 64 <= g.M)) {
    gemm_store_rows<true, true>(acc, g, row0, col0, lane);
  } else {
    gemm_store_rows<true, false>(acc, g, row0, col0, lane);
  }
}

// gemm_bf16x6_epi_kernel<EPI> below is a COPY of this prologue and k-loop (only the epilogue differs): a change here
// goes there too.
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kGemmStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 1, wn = wave & 1;                 // this wave's 64 x 64 output block
  const int ntb = g.N / kGemmBN;
  const int mtb = static_cast<int>((g.M + kGemmBM - 1) / kGemmBM);
  // XCD remap (bijective for any grid): consecutive tiles -- the same A row band -- share an XCD's L2
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb = wg / ntb, nb = wg - mb * ntb;
  const long m0 = static_cast<long>(mb) * kGemmBM;
  const int n0 = nb * kGemmBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits 2 (row, 8-k chunk) pieces of A per k-step -- m-tiles 2*wave, 2*wave+1, row lane & 15,
  // chunk lane >> 4 -- and stages 3 x 16 B of packed B
  const float* arow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    long r = m0 + (2 * wave + j) * 16 + (lane & 15);
    r = r < g.M ? r : g.M - 1;
    arow[j] = g.A + r * g.lda + 8 * (lane >> 4);
  }
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kGemmNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2][2];
  auto load = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ra[j][0] = *reinterpret_cast<const f32x4*>(arow[j] + kt * kGemmBK);
      ra[j][1] = *reinterpret_cast<const f32x4*>(arow[j] + kt * kGemmBK + 4);
    }
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16, which is where bdst[p * kGemmThreads + tid] = bsrc[...] used to put it
  char* const bwave = smem + kGemmABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kGemmStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kGemmStage;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x8 p0, p1, p2;
      split8(ra[j][0], ra[j][1], p0, p1, p2);
      bf16x8* dst = reinterpret_cast<bf16x8*>(base) + (2 * wave + j) * 3 * 64 + lane;
      dst[0] = p0;
      dst[64] = p1;
      dst[128] = p2;
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kGemmBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kGemmStage) + wm * 4 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kGemmStage + kGemmABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][4], fb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[p][i] = sa[(i * 3 + p) * 64];
        fb[p][i] = sb[(i * 3 + p) * 64];
      }
    // small terms first; each product sweeps all 16 accumulators (independent MFMAs back to back)
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};
    // the split of step k+1 sits between the two halves: half a step of MFMAs covers the loads' latency, and its VALU
    // work fills the gaps of the second half
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // B pieces 0, 1 behind the 24th MFMA and piece 2 behind the 36th.  Stage cur ^ 1 was last read in the step
          // that the barrier above this one ended
          if (t * 16 + i * 4 + j + 1 == 2 * kWideLoadPair) {
            load_b(nxt, cur ^ 1, 0);
            load_b(nxt, cur ^ 1, 1);
          }
          if (t * 16 + i * 4 + j + 1 == 3 * kWideLoadPair) load_b(nxt, cur ^ 1, 2);
        }
    }
    // placement of the 7 global loads, as in the wide kernel: the two A pairs ahead of the first and behind the 12th MFMA
    // (group barriers: hints), B where the source has it; tests/test_gemm_lds_staging.py checks where they land
#pragma unroll
    for (int n = 0; n < (4 + kGemmBPieces + 1) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  // epilogue: accumulator register r of tile (i, j) is row lane & 15, column (lane >> 4) * 4 + r (operands swapped)
  gemm_store(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
}

// ---- wide-tile variant: 128 x 256 outputs per workgroup, half the in-loop split work per MFMA ---------------------
// A workgroup splits BM x 32 values of A per k-step for BM x BN outputs, so every A value is split by N / BN
// workgroups; the split is most of the loop's non-MFMA vector work.  With the tile turned on its side (8 waves as 2 along
// M x 4 along N, 64 x 64 each as above) a thread splits ONE (row, 8-k) piece of A per k-step instead of two and stages
// 6 x 16 B of packed B instead of 3.  Same LDS footprint (A 8 m-tiles x 3 planes + B 16 n-tiles x 3 planes = 72 KiB per
// stage), same 24 fragment reads and 96 MFMAs per wave and k-step, same grid size, same packed B (the 16 n-tiles x 3
// planes of a k-step are one contiguous 48 KiB run), same split, same product and k-step order: every output has the
// bits of gemm_bf16x6_kernel.  Needs N % 256 == 0.
constexpr int kWideBM = 128, kWideBN = 256;
constexpr int kWideMT = kWideBM / 16, kWideNT = kWideBN / 16;          // 8 m-tiles, 16 n-tiles per workgroup
constexpr int kWideABytes = kWideMT * 3 * kTileBytes;                  // 24 KiB
constexpr int kWideBBytes = kWideNT * 3 * kTileBytes;                  // 48 KiB
constexpr int kWideStage = kWideABytes + kWideBBytes;                  // 72 KiB
constexpr int kWideBPieces = kWideBBytes / 16 / kGemmThreads;          // 6 x 16 B of B per thread and k-step

// gemm_bf16x6_wide_epi_kernel<EPI> below is a COPY of this prologue and k-loop (only the epilogue differs): a change
// here goes there too.
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_wide_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kWideStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 2, wn = wave & 3;                 // this wave's 64 x 64 output block
  const int ntb = g.N / kWideBN;
  const int mtb = static_cast<int>((g.M + kWideBM - 1) / kWideBM);
  // XCD remap as above
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb = wg / ntb, nb = wg - mb * ntb;
  const long m0 = static_cast<long>(mb) * kWideBM;
  const int n0 = nb * kWideBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and stages 6 x 16 B of packed B
  long r = m0 + wave * 16 + (lane & 15);
  r = r < g.M ? r : g.M - 1;
  const float* arow = g.A + r * g.lda + 8 * (lane >> 4);
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kWideNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2];
  auto load = [&](int kt) {
    ra[0] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK);
    ra[1] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK + 4);
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16, which is where bdst[p * kGemmThreads + tid] = bsrc[...] used to put it
  char* const bwave = smem + kWideABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kWideStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kWideStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kWideBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage) + wm * 4 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage + kWideABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][4], fb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[p][i] = sa[(i * 3 + p) * 64];
        fb[p][i] = sb[(i * 3 + p) * 64];
      }
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // a pair of B pieces behind every kWideLoadPair MFMAs of the first half.  Stage cur ^ 1 was last read in
          // the step that the barrier above this one ended
          if ((t * 16 + i * 4 + j + 1) % kWideLoadPair == 0 && (t * 16 + i * 4 + j + 1) / kWideLoadPair <= kWideBPieces / 2) {
            const int pair = (t * 16 + i * 4 + j + 1) / kWideLoadPair - 1;
            load_b(nxt, cur ^ 1, 2 * pair);
            load_b(nxt, cur ^ 1, 2 * pair + 1);
          }
        }
    }
    // placement of the 8 global loads: a pair per kWideLoadPair MFMAs over the first half of the step (the A pair
    // first; the split needs it).  Measured 5.7-7.6 % faster than all eight ahead of the first MFMA
    // (profiles/r10/README.md); that is consistent with every wave of the workgroup waiting in the vector-memory issue
    // queue right after the barrier before any of them reaches its MFMAs, which was not measured directly.  The direct
    // loads of B stay where the source has them (behind the 12th, 24th and 36th MFMA); the group barriers place the A
    // pair and keep the MFMAs from moving across the others.  They are hints: tests/test_gemm_wide.py and
    // tests/test_gemm_lds_staging.py check where the loads land
#pragma unroll
    for (int n = 0; n < (2 + kWideBPieces) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  // epilogue: accumulator register r of tile (i, j) is row lane & 15, column (lane >> 4) * 4 + r (operands swapped)
  gemm_store(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
}

// ---- GELU in the epilogue: the FFN's activation, or the product with its derivative, on the accumulators --------------
// gemm_bf16x6_epi_kernel<EPI> / gemm_bf16x6_wide_epi_kernel<EPI> are gemm_bf16x6_kernel / gemm_bf16x6_wide_kernel up to
// the epilogue, as copies: the prologue and the k-loop are the same text, so the same split, packed B, product and
// k-step order and (wide) load placement, and the unfused kernels' code objects do not change by a single instruction
// (a shared __device__ body changed their prologue scheduling and LDS addressing).  tests/test_gemm_epilogue.py holds
// the copies to the originals' loop budgets and to the bits of the unfused pair.

// The third epilogue of the two kernels below, behind an entry point of its own (vqa_gemm_bf16x6_lse): not a value of
// vqa_gemm_bf16x6_epi's `epilogue` argument, so the header does not define it.
#define VQA_GEMM_EPI_LSE 3

struct GemmEpiArgs : GemmArgs {
  float* aux;          // GELU: where the pre-activation goes (nullable); GELU_GRAD: the pre-activation (read only)
  long ldaux;
  // VQA_GEMM_EPI_LSE only (C, aux unused; vec = the bias may be read 16 bytes at a time)
  const int64_t* targets;   // [M]
  f32x2* part;              // [N / 64][M] (max, sum exp(x - max)) of a row's 64 columns
  float* tgt;               // [M] the logit at targets[row]
  int n_valid;              // columns >= n_valid are padding: masked to -inf
};

// What a wave does with its 64 x 64 block of accumulators at (row0, col0), on the transposed map of gemm_store_rows:
// register r of tile (i, j) is row i * 16 + (lane & 15), column j * 16 + (lane >> 4) * 4 + r.  Rows >= M are neither
// stored nor loaded from aux.
//   VQA_GEMM_EPI_GELU       h = acc (+ bias);  aux = h where aux is given;  C = gelu(h)
//   VQA_GEMM_EPI_GELU_GRAD  C = (acc (+ bias)) * gelu'(aux)
// GELU and its derivative are gelu.hpp's, on the pairs (0, 1) and (2, 3) of a tile's registers -- neighbouring columns;
// both are elementwise, so these are the bits of vqa_gelu_fwd / vqa_gelu_bwd applied to the plain epilogue's output.
// A tile's four values of h, aux and C are one 16-byte access each (VEC) or four dwords, and the tiles go row group by
// row group (i outer, j inner), so the four accesses of a row cover its 256 bytes -- two whole 128-byte lines -- back to
// back.  Column tile by column tile, where the other half of a line follows four (GELU with h stored: eight) stores
// later, the 16-byte form measured 1-2 % SLOWER than the dword stores it replaces in the GELU kernel and no faster in
// the GELU' kernel; row by row it is 2-3 % and 1-2 % faster (profiles/r13/README.md).  FULL: all 64 rows are below
// M, so nothing is guarded and the code is one basic block (behind a per-row branch the compiler waits for EVERY
// outstanding load, which serialises the h loads of GELU_GRAD with the arithmetic).
template <int EPI, bool FULL, bool VEC>
__device__ __forceinline__ void gemm_epilogue_rows(const f32x4 (&acc)[4][4], const GemmEpiArgs& g, long row0, int col0,
                                                   int lane) {
  const int colq = col0 + (lane >> 4) * 4;
  // acc (+ bias) of all 16 tiles ahead of the first store and the first h load, as in gemm_store_rows
  f32x4 v[4][4];
  if (g.bias) {
    f32x4 bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = load4<VEC>(g.bias + colq + j * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j] + bv[j];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j];
  }
  if constexpr (EPI == VQA_GEMM_EPI_GELU) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = colq + j * 16;
        const f32x4 h = v[i][j];
        const f32x2 lo = gelu2(f32x2{h.x, h.y}), hi = gelu2(f32x2{h.z, h.w});
        if (FULL || row < g.M) {
          if (g.aux) store4<VEC>(g.aux + row * g.ldaux + col, h);
          store4<VEC>(g.C + row * g.ldc + col, f32x4{lo.x, lo.y, hi.x, hi.y});
        }
      }
    }
  } else {
    // row group by row group, as above; the loads of row group i + 1 -- whole 128-byte lines of h -- are issued ahead
    // of the arithmetic of group i (the loop's prefetch and fragment registers are dead here: 2 x 16 registers of h fit)
    f32x4 hv[2][4];
    auto fetch = [&](int i, f32x4 (&dst)[4]) {
      const long row = row0 + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        dst[j] = (FULL || row < g.M) ? load4<VEC>(g.aux + row * g.ldaux + colq + j * 16) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    };
    fetch(0, hv[0]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i + 1 < 4) fetch(i + 1, hv[(i + 1) & 1]);
      const long row = row0 + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 d = v[i][j];
        const f32x4 h = hv[i & 1][j];
        const f32x2 lo = f32x2{d.x, d.y} * gelu_grad2(f32x2{h.x, h.y});
        const f32x2 hi = f32x2{d.z, d.w} * gelu_grad2(f32x2{h.z, h.w});
        if (FULL || row < g.M) store4<VEC>(g.C + row * g.ldc + colq + j * 16, f32x4{lo.x, lo.y, hi.x, hi.y});
      }
    }
  }
}

// ---- row log-sum-exp in the epilogue: an LM head's cross entropy without its [M, V] logits ------------------------------
// VQA_GEMM_EPI_LSE stores no C.  With x = acc (+ bias) on the map above and columns >= n_valid masked to -inf, a wave
// reduces each of its 64 rows over its 64 columns to (m, s) = (max x, sum exp(x - m)) and stores the pair to
// part[col0 / 64][row]; lse_combine_kernel folds a row's N / 64 pairs in block order.  A lane holds 16 of a row's values
// (4 tiles x 4 registers); the other 48 sit in the lanes with the same lane & 15, which v_permlane16_swap and
// v_permlane32_swap reach in two steps: with both operands the same register, the swap leaves (even 16-lane rows, odd
// rows) resp. (lower half, upper half) duplicated in its two results, and max / + of the two is the same value in the
// same order in every lane.  The maximum is reduced first and the exponentials are taken against the row's maximum of
// the block: 64 v_exp_f32 per lane and no rescaling.  Lane l then keeps row l (row group l >> 4), so the pairs leave as
// one 512-byte run of 8-byte stores per wave.  A block without a finite value (all -inf, or all padding) gives
// (-inf, 0): exp is taken against 0 there, not against -inf.  A NaN among a row's values makes s NaN; m skips it.
// The lane that holds column targets[row] stores that x -- the bits the plain epilogue would have put at
// C[row, target] -- to tgt[row]: one writer per row over the whole grid.  Both large tiles give a wave a 64 x 64 block
// at a multiple of 64, so they write the same pairs.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// The two results are read as .x / .y of a non-const vector: through __builtin_bit_cast(float, r[1]) of a const one the
// compiler handed out element 0 twice (profiles/r14/README.md).
__device__ __forceinline__ float lse_swap16(float v, bool is_max) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  u32x2 r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned ua = r.x, ub = r.y;
  const float a = __builtin_bit_cast(float, ua), b = __builtin_bit_cast(float, ub);
  return is_max ? fmaxf(a, b) : a + b;
}
__device__ __forceinline__ float lse_swap32(float v, bool is_max) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  u32x2 r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned ua = r.x, ub = r.y;
  const float a = __builtin_bit_cast(float, ua), b = __builtin_bit_cast(float, ub);
  return is_max ? fmaxf(a, b) : a + b;
}

__device__ __forceinline__ void gemm_epilogue_lse(const f32x4 (&acc)[4][4], const GemmEpiArgs& g, long row0, int col0,
                                                  int lane) {
  const int colq = col0 + (lane >> 4) * 4;
  // every load -- the bias and the four targets of this lane's rows (clamped like the rows of A) -- ahead of the
  // first store, as in gemm_store_rows
  f32x4 bv[4];
  if (g.bias) {
    if (g.vec) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = load4<true>(g.bias + colq + j * 16);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = load4<false>(g.bias + colq + j * 16);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  int tcol[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long row = row0 + i * 16 + (lane & 15);
    row = row < g.M ? row : g.M - 1;
    const long t = g.targets[row];
    tcol[i] = (t >= 0 && t < g.n_valid) ? static_cast<int>(t) : -1;     // ignore_index / a bad label: nobody writes tgt
  }
  const bool add_bias = g.bias != nullptr;
  const float ninf = -__builtin_inff();
  float mrow[4], srow[4], tval[4];
  bool mine[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float x[4][4];
    float m = ninf;
    tval[i] = 0.0f, mine[i] = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = colq + j * 16 + r;
        const float v = add_bias ? acc[i][j][r] + bv[j][r] : acc[i][j][r];
        if (col == tcol[i]) tval[i] = v, mine[i] = true;
        x[j][r] = col < g.n_valid ? v : ninf;
        m = fmaxf(m, x[j][r]);
      }
    m = lse_swap32(lse_swap16(m, true), true);
    const float ref = m == ninf ? 0.0f : m;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) s += __expf(x[j][r] - ref);
    s = lse_swap32(lse_swap16(s, false), false);
    mrow[i] = m, srow[i] = s;
  }
  // the stores behind the last use of a loaded value (one memory counter)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = row0 + i * 16 + (lane & 15);
    if (mine[i] && row < g.M) g.tgt[row] = tval[i];
  }
  const int grp = lane >> 4;
  const float mo = grp == 0 ? mrow[0] : grp == 1 ? mrow[1] : grp == 2 ? mrow[2] : mrow[3];
  const float so = grp == 0 ? srow[0] : grp == 1 ? srow[1] : grp == 2 ? srow[2] : srow[3];
  const long row = row0 + lane;                         // = row0 + grp * 16 + (lane & 15)
  if (row < g.M) g.part[static_cast<long>(col0 >> 6) * g.M + row] = f32x2{mo, so};
}

// The scalar path (a misaligned pointer or an odd stride) need not be fast: it has the guarded form only.
template <int EPI>
__device__ __forceinline__ void gemm_epilogue(const f32x4 (&acc)[4][4], const GemmEpiArgs& g, long row0, int col0,
                                              int lane) {
  if constexpr (EPI == VQA_GEMM_EPI_LSE) {
    gemm_epilogue_lse(acc, g, row0, col0, lane);
  } else if (!g.vec) {
    gemm_epilogue_rows<EPI, false, false>(acc, g, row0, col0, lane);
  } else if (__builtin_amdgcn_readfirstlane(row0 + 64 <= g.M)) {       // row0 is the wave's: uniform
    gemm_epilogue_rows<EPI, true, true>(acc, g, row0, col0, lane);
  } else {
    gemm_epilogue_rows<EPI, false, true>(acc, g, row0, col0, lane);
  }
}

template <int EPI>
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_epi_kernel(GemmEpiArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kGemmStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 1, wn = wave & 1;                 // this wave's 64 x 64 output block
  const int ntb = g.N / kGemmBN;
  const int mtb = static_cast<int>((g.M + kGemmBM - 1) / kGemmBM);
  // XCD remap (bijective for any grid): consecutive tiles -- the same A row band -- share an XCD's L2
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb = wg / ntb, nb = wg - mb * ntb;
  const long m0 = static_cast<long>(mb) * kGemmBM;
  const int n0 = nb * kGemmBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits 2 (row, 8-k chunk) pieces of A per k-step -- m-tiles 2*wave, 2*wave+1, row lane & 15,
  // chunk lane >> 4 -- and stages 3 x 16 B of packed B
  const float* arow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    long r = m0 + (2 * wave + j) * 16 + (lane & 15);
    r = r < g.M ? r : g.M - 1;
    arow[j] = g.A + r * g.lda + 8 * (lane >> 4);
  }
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kGemmNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2][2];
  auto load = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ra[j][0] = *reinterpret_cast<const f32x4*>(arow[j] + kt * kGemmBK);
      ra[j][1] = *reinterpret_cast<const f32x4*>(arow[j] + kt * kGemmBK + 4);
    }
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16, which is where bdst[p * kGemmThreads + tid] = bsrc[...] used to put it
  char* const bwave = smem + kGemmABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kGemmStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kGemmStage;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x8 p0, p1, p2;
      split8(ra[j][0], ra[j][1], p0, p1, p2);
      bf16x8* dst = reinterpret_cast<bf16x8*>(base) + (2 * wave + j) * 3 * 64 + lane;
      dst[0] = p0;
      dst[64] = p1;
      dst[128] = p2;
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kGemmBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kGemmStage) + wm * 4 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kGemmStage + kGemmABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][4], fb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[p][i] = sa[(i * 3 + p) * 64];
        fb[p][i] = sb[(i * 3 + p) * 64];
      }
    // small terms first; each product sweeps all 16 accumulators (independent MFMAs back to back)
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};
    // the split of step k+1 sits between the two halves: half a step of MFMAs covers the loads' latency, and its VALU
    // work fills the gaps of the second half
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // B pieces 0, 1 behind the 24th MFMA and piece 2 behind the 36th.  Stage cur ^ 1 was last read in the step
          // that the barrier above this one ended
          if (t * 16 + i * 4 + j + 1 == 2 * kWideLoadPair) {
            load_b(nxt, cur ^ 1, 0);
            load_b(nxt, cur ^ 1, 1);
          }
          if (t * 16 + i * 4 + j + 1 == 3 * kWideLoadPair) load_b(nxt, cur ^ 1, 2);
        }
    }
    // placement of the 7 global loads, as in the wide kernel: the two A pairs ahead of the first and behind the 12th MFMA
    // (group barriers: hints), B where the source has it; tests/test_gemm_lds_staging.py checks where they land
#pragma unroll
    for (int n = 0; n < (4 + kGemmBPieces + 1) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  gemm_epilogue<EPI>(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
}

template <int EPI>
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_wide_epi_kernel(GemmEpiArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kWideStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 2, wn = wave & 3;                 // this wave's 64 x 64 output block
  const int ntb = g.N / kWideBN;
  const int mtb = static_cast<int>((g.M + kWideBM - 1) / kWideBM);
  // XCD remap as above
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb = wg / ntb, nb = wg - mb * ntb;
  const long m0 = static_cast<long>(mb) * kWideBM;
  const int n0 = nb * kWideBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and stages 6 x 16 B of packed B
  long r = m0 + wave * 16 + (lane & 15);
  r = r < g.M ? r : g.M - 1;
  const float* arow = g.A + r * g.lda + 8 * (lane >> 4);
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kWideNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2];
  auto load = [&](int kt) {
    ra[0] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK);
    ra[1] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK + 4);
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16, which is where bdst[p * kGemmThreads + tid] = bsrc[...] used to put it
  char* const bwave = smem + kWideABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kWideStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kWideStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kWideBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage) + wm * 4 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage + kWideABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][4], fb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[p][i] = sa[(i * 3 + p) * 64];
        fb[p][i] = sb[(i * 3 + p) * 64];
      }
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // a pair of B pieces behind every kWideLoadPair MFMAs of the first half.  Stage cur ^ 1 was last read in
          // the step that the barrier above this one ended
          if ((t * 16 + i * 4 + j + 1) % kWideLoadPair == 0 && (t * 16 + i * 4 + j + 1) / kWideLoadPair <= kWideBPieces / 2) {
            const int pair = (t * 16 + i * 4 + j + 1) / kWideLoadPair - 1;
            load_b(nxt, cur ^ 1, 2 * pair);
            load_b(nxt, cur ^ 1, 2 * pair + 1);
          }
        }
    }
    // placement of the 8 global loads: a pair per kWideLoadPair MFMAs over the first half of the step (the A pair
    // first; the split needs it).  Measured 5.7-7.6 % faster than all eight ahead of the first MFMA
    // (profiles/r10/README.md); that is consistent with every wave of the workgroup waiting in the vector-memory issue
    // queue right after the barrier before any of them reaches its MFMAs, which was not measured directly.  The direct
    // loads of B stay where the source has them (behind the 12th, 24th and 36th MFMA); the group barriers place the A
    // pair and keep the MFMAs from moving across the others.  They are hints: tests/test_gemm_wide.py and
    // tests/test_gemm_lds_staging.py check where the loads land
#pragma unroll
    for (int n = 0; n < (2 + kWideBPieces) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  gemm_epilogue<EPI>(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
}

// ---- grouped launch: the 128 x 256 tiles of up to four (A, packed B, C) problems with one (N, K) in ONE grid ---------
// A mixture-of-experts FFN runs the same (N, K) product on several row sets with a weight each.  The large tiles run one
// workgroup per CU, so every launch ends in a round that is partly empty, and a small problem (VLMo's text expert:
// 7 m-blocks beside the image expert's 289) cannot fill the device by itself at all.  gemm_bf16x6_grouped_kernel<EPI>
// puts the tiles of all groups into one list -- the m-blocks of group 0, then those of group 1, ..., within an m-block
// the N / 256 column blocks as in gemm_bf16x6_wide_kernel -- and applies that kernel's XCD remap to the combined list.
// The groups travel BY VALUE in the kernel arguments (no device-side table, no allocation, no copy: the launch is
// graph-capturable); a workgroup compares its m-block against the cumulative block counts (blockIdx arithmetic: scalar
// registers) and takes that group's pointers, strides and M.  A group with M == 0 has no m-block.  From there on it is
// gemm_bf16x6_wide_epi_kernel up to the epilogue, as a copy (see the note above GemmEpiArgs): rows >= M of the GROUP
// are read clamped to the group's row M - 1 and never stored; same split, packed B, load placement, product and k-step
// order, so every output has the bits of the wide kernel run on its group alone.  EPI == 0 ends in gemm_store, the
// others in gemm_epilogue<EPI>, on a per-group argument block built in registers.  One `vec` serves the launch: set
// only where every group with rows passes gemm_vec_ok.
struct GemmGroup {
  const float* A;
  const bf16x8* B;     // packed planes
  const float* bias;   // nullable
  float* C;
  float* aux;          // as GemmEpiArgs::aux
  long lda, ldc, ldaux, M;
};

struct GemmGroupedArgs {
  GemmGroup grp[VQA_GEMM_MAX_GROUPS];
  int start[VQA_GEMM_MAX_GROUPS + 1];   // start[i] = m-blocks of the groups ahead of group i; start[4] = all of them
  int N, K;
  int vec;
};

template <int EPI>
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_grouped_kernel(GemmGroupedArgs ga) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kWideStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 2, wn = wave & 3;                 // this wave's 64 x 64 output block
  const int ntb = ga.N / kWideBN;
  const int mtb = ga.start[VQA_GEMM_MAX_GROUPS];
  // XCD remap as above, over the combined list
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb_all = wg / ntb, nb = wg - mb_all * ntb;
  // the group of this m-block: the last one whose first block is not behind it (an empty group shares its successor's
  // start and is skipped; groups behind the last one with rows start at mtb, which no m-block reaches)
  const int gi = (mb_all >= ga.start[1]) + (mb_all >= ga.start[2]) + (mb_all >= ga.start[3]);
  const GemmGroup& grp = ga.grp[gi];
  GemmEpiArgs g;
  g.A = grp.A, g.B = grp.B, g.bias = grp.bias, g.C = grp.C;
  g.lda = grp.lda, g.ldc = grp.ldc, g.M = grp.M;
  g.N = ga.N, g.K = ga.K, g.vec = ga.vec;
  g.aux = grp.aux, g.ldaux = grp.ldaux;
  const int mb = mb_all - ga.start[gi];
  const long m0 = static_cast<long>(mb) * kWideBM;
  const int n0 = nb * kWideBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and stages 6 x 16 B of packed B
  long r = m0 + wave * 16 + (lane & 15);
  r = r < g.M ? r : g.M - 1;
  const float* arow = g.A + r * g.lda + 8 * (lane >> 4);
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kWideNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2];
  auto load = [&](int kt) {
    ra[0] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK);
    ra[1] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK + 4);
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16, which is where bdst[p * kGemmThreads + tid] = bsrc[...] used to put it
  char* const bwave = smem + kWideABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kWideStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kWideStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kWideBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage) + wm * 4 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage + kWideABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][4], fb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        fa[p][i] = sa[(i * 3 + p) * 64];
        fb[p][i] = sb[(i * 3 + p) * 64];
      }
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // a pair of B pieces behind every kWideLoadPair MFMAs of the first half.  Stage cur ^ 1 was last read in
          // the step that the barrier above this one ended
          if ((t * 16 + i * 4 + j + 1) % kWideLoadPair == 0 && (t * 16 + i * 4 + j + 1) / kWideLoadPair <= kWideBPieces / 2) {
            const int pair = (t * 16 + i * 4 + j + 1) / kWideLoadPair - 1;
            load_b(nxt, cur ^ 1, 2 * pair);
            load_b(nxt, cur ^ 1, 2 * pair + 1);
          }
        }
    }
    // placement of the 8 global loads: as in gemm_bf16x6_wide_kernel (a pair per kWideLoadPair MFMAs over the first
    // half of the step, the A pair first)
#pragma unroll
    for (int n = 0; n < (2 + kWideBPieces) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  // rows and M are the group's own: the FULL form runs for a wave whose 64 rows are all below its group's M
  if constexpr (EPI == VQA_GEMM_EPI_NONE) {
    gemm_store(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
  } else {
    gemm_epilogue<EPI>(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
  }
}

// ---- persistent launch of the 128 x 256 tile: one workgroup per CU walks a list of tiles -----------------------------
// At 144 KiB of LDS a large tile is alone on its CU, so nothing covers what a tile pays once: the wait for its first
// operands (global loads, the split, a barrier) with the matrix pipe idle.  gemm_bf16x6_persistent_kernel is
// gemm_bf16x6_wide_kernel with a tile loop around its k-loop, as a copy (see the note above GemmEpiArgs), launched with
// `workgroups` <= tiles workgroups.  In a tile's LAST k-step -- where the wide kernel reloads the step it is running into
// the idle LDS buffer only to avoid a branch -- the loads fetch step 0 of the workgroup's next tile (its rows clamped to
// M - 1, its column block of packed B), so behind the barrier that ends the step the next tile's operands are staged
// and published: the wave stores its accumulators, zeroes them and goes straight into the next k-loop.  The buffer
// parity runs on across tiles (a tile with an odd number of k-steps hands over in the other buffer); with one k-step
// the only step is also the last.  The workgroup's last tile keeps the wide kernel's reload of itself, so nothing is
// read that the wide kernel would not read.
//
// Tile list: tiles are numbered m-block major, the N / 256 column blocks fastest, as in the wide kernel.  The XCD remap
// of the wide kernel, applied to the WORKGROUPS, gives the grid's workgroups an order in which those of one XCD are
// neighbours at positions [pos, pos + wx); the XCD's run of the tile list is [tiles * pos / W, tiles * (pos + wx) / W)
// -- ONE contiguous run per XCD, in proportion to its workgroups -- and they deal it out in turn: workgroup i of wx
// takes tiles i, i + wx, i + 2 wx, ... of the run.  At any time an XCD therefore works on a window of neighbouring tiles
// (the same rows of A, every column block of B), as a round of the wide kernel does, no workgroup has more than
// ceil(tiles / W) tiles, and the workgroups that have one tile more than the others are spread over all XCDs, as the
// part-filled last round of the wide kernel is.  (Cutting the list into W equal runs first puts those workgroups on
// the first XCDs, which then run their last tile as slowly as a full round: measured 3-10 % slower than the wide kernel,
// profiles/r17/README.md.)  The assignment is blockIdx arithmetic: no atomics, no counters, nothing to reset between
// launches (graph replay).  With workgroups <= tiles every workgroup has a tile; one without returns before it touches
// memory.
//
// Same split, packed B, load placement, product and k-step order per tile, and gemm_store: every output has the bits
// of gemm_bf16x6_wide_kernel.
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_persistent_kernel(GemmArgs g, int ntiles) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kWideStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 2, wn = wave & 3;                 // this wave's 64 x 64 output block
  const int ntb = g.N / kWideBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;
  // this workgroup's tiles: run0 + i, run0 + i + wx, ... below run1 (see above)
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wx = q + (xcd < rem ? 1 : 0);                                              // workgroups of this XCD
  const int pos = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;         // the first of them, remapped
  const int run0 = static_cast<int>(static_cast<long>(ntiles) * pos / nwg);
  const int run1 = static_cast<int>(static_cast<long>(ntiles) * (pos + wx) / nwg);
  int tile = run0 + (orig >> 3);
  if (tile >= run1) return;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and stages 6 x 16 B of packed B
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B
  // where tile t starts: its first row and column, this thread's row of A (step 0) and the tile's run of packed B
  auto locate = [&](int t, long& m0, int& n0, const float*& arow, const bf16x8*& bsrc) {
    const int mb = t / ntb, nb = t - mb * ntb;
    m0 = static_cast<long>(mb) * kWideBM;
    n0 = nb * kWideBN;
    long r = m0 + wave * 16 + (lane & 15);
    r = r < g.M ? r : g.M - 1;
    arow = g.A + r * g.lda + 8 * (lane >> 4);
    bsrc = g.B + static_cast<size_t>(nb) * kWideNT * 3 * 64;
  };
  long m0;
  int n0;
  const float* arow;
  const bf16x8* bsrc;
  locate(tile, m0, n0, arow, bsrc);

  f32x4 ra[2];
  auto load = [&](const float* src) {
    ra[0] = *reinterpret_cast<const f32x4*>(src);
    ra[1] = *reinterpret_cast<const f32x4*>(src + 4);
  };
  // piece p of the k-step of packed B at src into stage s, with no register in between: the wave's KiB lands at the
  // base given here + lane * 16
  char* const bwave = smem + kWideABytes + wave_u * kTileBytes;
  auto load_b = [&](const bf16x8* src, int s, int p) {
    stage_b16(src + p * kGemmThreads + tid, bwave + s * kWideStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kWideStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // the only prologue of the workgroup: step 0 of its first tile
  load(arow);
#pragma unroll
  for (int p = 0; p < kWideBPieces; ++p) load_b(bsrc, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  int cur = 0;                                   // the buffer that holds the step about to run: flips per k-step, across tiles
  for (;;) {
    // what the tile's last k-step loads: step 0 of the next tile, or (the workgroup's last tile) that step again
    const int tnext = tile + wx;
    const bool more = tnext < run1;
    long m0n = m0;
    int n0n = n0;
    const float* arow_n = arow + (nk - 1) * kGemmBK;
    const bf16x8* bsrc_n = bsrc + (nk - 1) * bstep;
    if (more) locate(tnext, m0n, n0n, arow_n, bsrc_n);
    // one k-step on the operands in buffer cur; anxt / bnxt: what it stages into the other buffer
    auto step = [&](const float* anxt, const bf16x8* bnxt) {
      load(anxt);
      const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage) + wm * 4 * 3 * 64 + lane;
      const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kWideStage + kWideABytes) + wn * 4 * 3 * 64 + lane;
      bf16x8 fa[3][4], fb[3][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          fa[p][i] = sa[(i * 3 + p) * 64];
          fb[p][i] = sb[(i * 3 + p) * 64];
        }
      constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        if (t == 3) store(cur ^ 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
            // a pair of B pieces behind every kWideLoadPair MFMAs of the first half.  Stage cur ^ 1 was last read in
            // the step that the barrier above this one ended -- of this tile or of the one before
            if ((t * 16 + i * 4 + j + 1) % kWideLoadPair == 0 && (t * 16 + i * 4 + j + 1) / kWideLoadPair <= kWideBPieces / 2) {
              const int pair = (t * 16 + i * 4 + j + 1) / kWideLoadPair - 1;
              load_b(bnxt, cur ^ 1, 2 * pair);
              load_b(bnxt, cur ^ 1, 2 * pair + 1);
            }
          }
      }
      // placement of the 8 global loads: as in gemm_bf16x6_wide_kernel (a pair per kWideLoadPair MFMAs over the first
      // half of the step, the A pair first)
#pragma unroll
      for (int n = 0; n < (2 + kWideBPieces) / 2; ++n) {
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
        __builtin_amdgcn_sched_group_barrier(0x008, kWideLoadPair, 0);      // kWideLoadPair MFMAs
      }
      stage_b_wait();
      __syncthreads();
      cur ^= 1;
    };
    // the wide kernel's loop over all steps but the last, which is the same step on other pointers: no select in the loop
    for (int kt = 0; kt + 1 < nk; ++kt) step(arow + (kt + 1) * kGemmBK, bsrc + (kt + 1) * bstep);
    step(arow_n, bsrc_n);

    // epilogue of the wide kernel.  The stores read registers only; the next tile's first step is already in LDS
    gemm_store(acc, g, m0 + wm * 64, n0 + wn * 64, lane);
    if (!more) break;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    tile = tnext, m0 = m0n, n0 = n0n, arow = arow_n, bsrc = bsrc_n;
  }
}

// ---- small-tile variant for grids the 256 x 128 tile cannot fill (a few hundred rows, or a narrow N) ---------------
// Same packed B, same split, same product and k-step order, so with ksplit == 1 every output has the bits of
// gemm_bf16x6_kernel.  Tile: 64 x 128 outputs per workgroup of 4 waves (2 along M x 2 along N, 32 x 64 each = 2 x 4 MFMA
// tiles), BK = 32.  LDS per k-step: A 4 m-tiles x 3 planes x 1 KiB + B 24 KiB = 36 KiB, double-buffered = 72 KiB (two
// workgroups per CU), fragment order as above.  Per k-step a wave issues 18 fragment reads and 48 MFMAs.
//
// Split-K: part p of ksplit covers the k-steps [p * nk / ksplit, (p + 1) * nk / ksplit) and, with ksplit > 1, stores its
// fp32 partial tile (no bias) to ws[p][M][N]; gemm_splitk_combine_kernel, launched behind it on the same stream, forms
// ((P0 + P1) + ... + P(ksplit-1)) + bias in that order.  No atomics, no counters: nothing depends on arrival order and
// nothing has to be reset between launches (graph replay).
constexpr int kSmallBM = 64;
constexpr int kSmallThreads = 256;
constexpr int kSmallMT = kSmallBM / 16;                                // 4 m-tiles per workgroup
constexpr int kSmallABytes = kSmallMT * 3 * kTileBytes;                // 12 KiB
constexpr int kSmallStage = kSmallABytes + kGemmBBytes;                // 36 KiB
constexpr int kSmallBPieces = kGemmBBytes / 16 / kSmallThreads;        // 6 x 16 B of B per thread and k-step
constexpr int kGemmMaxKSplit = 16;

__global__ __launch_bounds__(kSmallThreads) void gemm_bf16x6_small_kernel(GemmArgs g, float* __restrict__ ws, int ksplit) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kSmallStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;                 // this wave's 32 x 64 output block
  const int ntb = g.N / kGemmBN;
  const int mtb = static_cast<int>((g.M + kSmallBM - 1) / kSmallBM);
  const int tiles = mtb * ntb;
  // XCD remap as above; the part index is the slowest, so the tiles of one row band and part share an XCD's L2
  const int nwg = tiles * ksplit, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int part = wg / tiles, tile = wg - part * tiles;
  const int mb = tile / ntb, nb = tile - mb * ntb;
  const long m0 = static_cast<long>(mb) * kSmallBM;
  const int n0 = nb * kGemmBN;
  const int nk = g.K / kGemmBK;
  const int k0 = part * nk / ksplit, k1 = (part + 1) * nk / ksplit;    // ksplit <= nk: never empty
  const int nt16 = g.N / 16;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and copies 6 x 16 B of packed B
  long r = m0 + wave * 16 + (lane & 15);
  r = r < g.M ? r : g.M - 1;
  const float* arow = g.A + r * g.lda + 8 * (lane >> 4);
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kGemmNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2];
  bf16x8 rb[kSmallBPieces];
  auto load = [&](int kt) {
    ra[0] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK);
    ra[1] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK + 4);
#pragma unroll
    for (int p = 0; p < kSmallBPieces; ++p) rb[p] = bsrc[kt * bstep + p * kSmallThreads + tid];
  };
  auto store = [&](int s) {
    char* base = smem + s * kSmallStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
    bf16x8* bdst = reinterpret_cast<bf16x8*>(base + kSmallABytes);
#pragma unroll
    for (int p = 0; p < kSmallBPieces; ++p) bdst[p * kSmallThreads + tid] = rb[p];
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(k0);
  store(0);
  __syncthreads();
  for (int kt = k0; kt < k1; ++kt) {
    const int cur = (kt - k0) & 1;
    load(kt + 1 < k1 ? kt + 1 : kt);          // the last step reloads its own tile into the idle buffer: no branch
    __builtin_amdgcn_sched_barrier(0);        // keep the loads ahead of the MFMAs
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kSmallStage) + wm * 2 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kSmallStage + kSmallABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][2], fb[3][4];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[p][i] = sa[(i * 3 + p) * 64];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[p][j] = sb[(j * 3 + p) * 64];
    }
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kPa[t]][i], fb[kPb[t]][j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: accumulator register r of tile (i, j) is row (lane >> 4) * 4 + r, column lane & 15.  A part of a split
  // stores the bare accumulators into its [M, N] slab of the workspace
  float* out = ksplit == 1 ? g.C : ws + static_cast<size_t>(part) * g.M * g.N;
  const long ldo = ksplit == 1 ? g.ldc : g.N;
  const bool add_bias = ksplit == 1 && g.bias;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + wn * 64 + j * 16 + (lane & 15);
    const float bv = add_bias ? g.bias[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long row = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + rr;
        if (row < g.M) out[row * ldo + col] = add_bias ? acc[i][j][rr] + bv : acc[i][j][rr];
      }
  }
}

// ---- half tile: 128 x 128 outputs per workgroup, for the rows behind the last full round of a large-tile launch ------
// The 256 x 128 and 128 x 256 tiles run one workgroup per CU, so a launch proceeds in rounds of one tile per CU and its
// last round is as long as the others however few tiles it holds.  vqa_gemm_bf16x6_tail runs the rows of that round on
// this tile instead: twice as many workgroups of half the length, where they still fit one round.  Built like the two
// large tiles -- BK = 32, packed B straight into LDS (3 x 16 B per thread and k-step), A split on the fly (one
// (row, 8-k) piece per thread, as in the wide kernel), MFMA operands swapped so a lane holds four consecutive columns --
// with 8 waves as 4 along M x 2 along N, 32 x 64 outputs each = 2 x 4 MFMA tiles.  LDS per k-step: A 8 m-tiles x 3
// planes + B 8 n-tiles x 3 planes = 48 KiB, double-buffered = 96 KiB (one workgroup per CU).  Per k-step a wave issues
// 18 fragment reads and 48 MFMAs; the five global loads of the next step go out in the first half of them (the A pair
// ahead of the first MFMA, B pieces 0 and 1 behind the 6th, piece 2 behind the 12th).  Same split, packed B, product
// and k-step order: every output has the bits of the other kernels.  No split-K and no fused epilogue.  Its own copy
// of the loop, like the _epi kernels: the large tiles' code objects do not change.
constexpr int kHalfBM = 128;                                           // x kGemmBN = 128 columns
constexpr int kHalfMT = kHalfBM / 16;                                  // 8 m-tiles (and kGemmNT = 8 n-tiles) per workgroup
constexpr int kHalfABytes = kHalfMT * 3 * kTileBytes;                  // 24 KiB
constexpr int kHalfStage = kHalfABytes + kGemmBBytes;                  // 48 KiB
constexpr int kHalfLoadPair = 6;                                       // MFMAs behind each pair of global loads of the next step

// gemm_store_rows for a wave's 32 x 64 block: register r of tile (i, j), i < 2, is row i * 16 + (lane & 15), column
// j * 16 + (lane >> 4) * 4 + r.  The bias is added to all 8 tiles ahead of the first store, as there.
template <bool VEC, bool FULL>
__device__ __forceinline__ void gemm_store_rows_half(const f32x4 (&acc)[2][4], const GemmArgs& g, long row0, int col0, int lane) {
  const int colq = col0 + (lane >> 4) * 4;
  f32x4 v[2][4];
  if (g.bias) {
    f32x4 bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = load4<VEC>(g.bias + colq + j * 16);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j] + bv[j];
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = acc[i][j];
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long row = row0 + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (FULL || row < g.M) store4<VEC>(g.C + row * g.ldc + colq + j * 16, v[i][j]);
  }
}

__global__ __launch_bounds__(kGemmThreads) void gemm_bf16x6_half_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kHalfStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // the same value, known to be uniform
  const int wm = wave >> 1, wn = wave & 1;                 // this wave's 32 x 64 output block
  const int ntb = g.N / kGemmBN;
  const int mtb = static_cast<int>((g.M + kHalfBM - 1) / kHalfBM);
  // XCD remap as above
  const int nwg = mtb * ntb, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
  const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  const int mb = wg / ntb, nb = wg - mb * ntb;
  const long m0 = static_cast<long>(mb) * kHalfBM;
  const int n0 = nb * kGemmBN;
  const int nk = g.K / kGemmBK;
  const int nt16 = g.N / 16;

  // staging: this thread splits one (row, 8-k chunk) piece of A per k-step -- m-tile wave, row lane & 15, chunk
  // lane >> 4 -- and stages 3 x 16 B of packed B
  long r = m0 + wave * 16 + (lane & 15);
  r = r < g.M ? r : g.M - 1;
  const float* arow = g.A + r * g.lda + 8 * (lane >> 4);
  const bf16x8* bsrc = g.B + static_cast<size_t>(nb) * kGemmNT * 3 * 64;
  const size_t bstep = static_cast<size_t>(nt16) * 3 * 64;            // bf16x8 per k-step of packed B

  f32x4 ra[2];
  auto load = [&](int kt) {
    ra[0] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK);
    ra[1] = *reinterpret_cast<const f32x4*>(arow + kt * kGemmBK + 4);
  };
  // piece p of step kt's packed B into stage s, with no register in between: the wave's KiB lands at the base given
  // here + lane * 16 = byte (p * kGemmThreads + tid) * 16 of the stage's image of B
  char* const bwave = smem + kHalfABytes + wave_u * kTileBytes;
  auto load_b = [&](int kt, int s, int p) {
    stage_b16(bsrc + kt * bstep + p * kGemmThreads + tid, bwave + s * kHalfStage + p * kGemmThreads * 16);
  };
  auto store = [&](int s) {
    char* base = smem + s * kHalfStage;
    bf16x8 p0, p1, p2;
    split8(ra[0], ra[1], p0, p1, p2);
    bf16x8* dst = reinterpret_cast<bf16x8*>(base) + wave * 3 * 64 + lane;
    dst[0] = p0;
    dst[64] = p1;
    dst[128] = p2;
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(0);
#pragma unroll
  for (int p = 0; p < kGemmBPieces; ++p) load_b(0, 0, p);
  store(0);
  stage_b_wait();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const int nxt = kt + 1 < nk ? kt + 1 : kt;   // the last step reloads its own tile into the idle buffer: no branch
    load(nxt);
    const bf16x8* sa = reinterpret_cast<const bf16x8*>(smem + cur * kHalfStage) + wm * 2 * 3 * 64 + lane;
    const bf16x8* sb = reinterpret_cast<const bf16x8*>(smem + cur * kHalfStage + kHalfABytes) + wn * 4 * 3 * 64 + lane;
    bf16x8 fa[3][2], fb[3][4];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[p][i] = sa[(i * 3 + p) * 64];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[p][j] = sb[(j * 3 + p) * 64];
    }
    constexpr int kPa[6] = {2, 1, 0, 1, 0, 0}, kPb[6] = {0, 1, 2, 0, 1, 0};   // the order of gemm_bf16x6_kernel
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == 3) store(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kPb[t]][j], fa[kPa[t]][i], acc[i][j], 0, 0, 0);   // transposed
          // B pieces 0, 1 behind the 6th MFMA and piece 2 behind the 12th.  Stage cur ^ 1 was last read in the step
          // that the barrier above this one ended
          if (t * 8 + i * 4 + j + 1 == kHalfLoadPair) {
            load_b(nxt, cur ^ 1, 0);
            load_b(nxt, cur ^ 1, 1);
          }
          if (t * 8 + i * 4 + j + 1 == 2 * kHalfLoadPair) load_b(nxt, cur ^ 1, 2);
        }
    }
    // placement of the 5 global loads, as in the large tiles: the A pair ahead of the first MFMA (group barriers:
    // hints), B where the source has it; tests/test_gemm_tail.py checks where they land
#pragma unroll
    for (int n = 0; n < (2 + kGemmBPieces + 1) / 2; ++n) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                  // two vector-memory reads
      __builtin_amdgcn_sched_group_barrier(0x008, kHalfLoadPair, 0);      // kHalfLoadPair MFMAs
    }
    stage_b_wait();
    __syncthreads();
  }

  // epilogue: accumulator register r of tile (i, j) is row lane & 15, column (lane >> 4) * 4 + r (operands swapped).
  // The vector form unguarded where all 32 rows of the wave's block are below M (row0 is the wave's: uniform)
  const long row0 = m0 + wm * 32;
  const int col0 = n0 + wn * 64;
  if (!g.vec) {
    gemm_store_rows_half<false, false>(acc, g, row0, col0, lane);
  } else if (__builtin_amdgcn_readfirstlane(row0 + 32 <= g.M)) {
    gemm_store_rows_half<true, true>(acc, g, row0, col0, lane);
  } else {
    gemm_store_rows_half<true, false>(acc, g, row0, col0, lane);
  }
}

// C = ((P0 + P1) + ... + P(ksplit-1)) + bias over the [ksplit][M][N] partials, one thread per 4 columns of a row.
__global__ __launch_bounds__(kBlock) void gemm_splitk_combine_kernel(const f32x4* __restrict__ ws,
                                                                     const float* __restrict__ bias, float* __restrict__ C,
                                                                     long ldc, long M, int N, int ksplit, int vec) {
  const int n4 = N / 4;
  const long total = M * n4;
  for (long idx = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long>(gridDim.x) * blockDim.x) {
    f32x4 s = ws[idx];
    for (int p = 1; p < ksplit; ++p) s = s + ws[p * total + idx];
    const long row = idx / n4;
    const int col = static_cast<int>(idx - row * n4) * 4;
    if (bias) s = s + f32x4{bias[col], bias[col + 1], bias[col + 2], bias[col + 3]};
    float* dst = C + row * ldc + col;
    if (vec) {
      *reinterpret_cast<f32x4*>(dst) = s;
    } else {
      dst[0] = s.x, dst[1] = s.y, dst[2] = s.z, dst[3] = s.w;
    }
  }
}

// Folds a row's N / 64 (max, sum) pairs in block order, one row per lane (consecutive lanes read consecutive pairs of a
// block): (mx, sm) <- (max(mx, m), sm * exp(mx - max) + s * exp(m - max)); nothing is rescaled while the running maximum
// is still -inf (exp(-inf - -inf) would be NaN), and a NaN sum stays NaN.  lse = mx + log(sm);
// row_loss = log(sm) - (tgt - mx): lse - tgt without rounding at ulp(mx) first (as vqa_ce_rows forms it).
__global__ __launch_bounds__(kBlock) void lse_combine_kernel(const f32x2* __restrict__ part, const float* __restrict__ tgt,
                                                             const int64_t* __restrict__ targets, long ignore_index,
                                                             long M, int nblk, int n_valid, float* __restrict__ row_loss,
                                                             float* __restrict__ lse, int* __restrict__ flag) {
  const float ninf = -__builtin_inff();
  for (long row = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x; row < M;
       row += static_cast<long>(gridDim.x) * blockDim.x) {
    float mx = ninf, sm = 0.0f;
    for (int b = 0; b < nblk; ++b) {
      const f32x2 p = part[static_cast<long>(b) * M + row];
      const float nm = fmaxf(mx, p.x);
      if (nm == ninf) {
        sm += p.y;                                      // 0, or the NaN of a block that met one
      } else {
        sm = sm * __expf(mx - nm) + p.y * __expf(p.x - nm);
        mx = nm;
      }
    }
    const float ls = logf(sm);
    if (lse) lse[row] = mx + ls;
    const long t = targets[row];
    float loss = 0.0f;
    if (t != ignore_index) {
      if (t >= 0 && t < n_valid) {
        loss = ls - (tgt[row] - mx);
      } else {
        loss = __builtin_nanf("");
        if (flag) atomicOr(flag, VQA_FLAG_BAD_LABEL);
      }
    }
    row_loss[row] = loss;
  }
}

// One thread per (k-tile, n-tile, lane): 8 consecutive k of one column, split into the three planes.
__global__ __launch_bounds__(kBlock) void gemm_pack_b_kernel(const float* __restrict__ w, long ldw, int trans,
                                                             bf16x8* __restrict__ out, int K, int N) {
  const long total = static_cast<long>(K / 32) * (N / 16) * 64;
  for (long idx = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<long>(gridDim.x) * blockDim.x) {
    const int l = static_cast<int>(idx & 63);
    const long tile = idx >> 6;                           // kt * (N / 16) + nt
    const int nt = static_cast<int>(tile % (N / 16)), kt = static_cast<int>(tile / (N / 16));
    const int n = nt * 16 + (l & 15), k = kt * 32 + 8 * (l >> 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = trans ? w[static_cast<long>(n) * ldw + k + e] : w[static_cast<long>(k + e) * ldw + n];
    bf16x8 p0, p1, p2;
    split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, p0, p1, p2);
    out[(tile * 3 + 0) * 64 + l] = p0;
    out[(tile * 3 + 1) * 64 + l] = p1;
    out[(tile * 3 + 2) * 64 + l] = p2;
  }
}

}  // namespace vqa

using namespace vqa;

// The large-tile kernels' vector epilogue: every pointer it touches on a 16-byte boundary, every row stride it steps by a
// multiple of 4 floats (columns start at multiples of 4).  Anything else runs the same lane map with dword accesses.
static int gemm_vec_ok(const float* C, long ldc, const float* bias, const float* aux = nullptr, long ldaux = 0) {
  return aligned16(C) && ldc % 4 == 0 && (!bias || aligned16(bias)) && (!aux || (aligned16(aux) && ldaux % 4 == 0));
}

extern "C" {

size_t vqa_gemm_packed_bytes(int K, int N) {
  if (K <= 0 || N <= 0 || K % kGemmBK || N % kGemmBN) return 0;
  return static_cast<size_t>(K) * N * 3 * sizeof(__bf16);
}

int vqa_gemm_pack_b(const float* w, long ldw, int trans, void* packed, int K, int N, vqa_stream_t stream) {
  clear_stale_error();
  if (!w || !packed) return VQA_ERR_NULL;
  if (K <= 0 || N <= 0 || K % kGemmBK || N % kGemmBN || (trans != 0 && trans != 1)) return VQA_ERR_SHAPE;
  if (ldw < (trans ? K : N)) return VQA_ERR_SHAPE;
  if (!aligned4(w) || !aligned16(packed)) return VQA_ERR_ALIGN;
  const long work = static_cast<long>(K / 32) * (N / 16) * 64;
  gemm_pack_b_kernel<<<blocks_for(work, kBlock), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      w, ldw, trans, static_cast<bf16x8*>(packed), K, N);
  return launch_status();
}

int vqa_gemm_bf16x6(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M, int N,
                    int K, vqa_stream_t stream) {
  clear_stale_error();
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if ((M + kGemmBM - 1) / kGemmBM * (N / kGemmBN) > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  GemmArgs g{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K, gemm_vec_ok(C, ldc, bias)};
  const int grid = static_cast<int>((M + kGemmBM - 1) / kGemmBM * (N / kGemmBN));
  gemm_bf16x6_kernel<<<grid, kGemmThreads, 0, static_cast<hipStream_t>(stream)>>>(g);
  return launch_status();
}

int vqa_gemm_bf16x6_tile(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, int tile, vqa_stream_t stream) {
  if (tile != VQA_GEMM_TILE_256X128 && tile != VQA_GEMM_TILE_128X256) {
    clear_stale_error();
    return VQA_ERR_SHAPE;
  }
  // the wide tile stages 16 n-tiles per workgroup: every other N runs the 256 x 128 kernel (same bits)
  if (tile == VQA_GEMM_TILE_256X128 || N <= 0 || N % kWideBN) return vqa_gemm_bf16x6(A, lda, packed, bias, C, ldc, M, N, K, stream);
  clear_stale_error();
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || K <= 0 || K % kGemmBK || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if ((M + kWideBM - 1) / kWideBM * (N / kWideBN) > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  GemmArgs g{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K, gemm_vec_ok(C, ldc, bias)};
  const int grid = static_cast<int>((M + kWideBM - 1) / kWideBM * (N / kWideBN));
  gemm_bf16x6_wide_kernel<<<grid, kGemmThreads, 0, static_cast<hipStream_t>(stream)>>>(g);
  return launch_status();
}

int vqa_gemm_bf16x6_persistent(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                               int N, int K, int workgroups, vqa_stream_t stream) {
  clear_stale_error();
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kWideBN || lda < K || lda % 4 || ldc < N || workgroups < 1) return VQA_ERR_SHAPE;
  if ((M + kWideBM - 1) / kWideBM * (N / kWideBN) > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  GemmArgs g{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K, gemm_vec_ok(C, ldc, bias)};
  const int ntiles = static_cast<int>((M + kWideBM - 1) / kWideBM * (N / kWideBN));
  const int grid = workgroups < ntiles ? workgroups : ntiles;          // every workgroup has a tile
  gemm_bf16x6_persistent_kernel<<<grid, kGemmThreads, 0, static_cast<hipStream_t>(stream)>>>(g, ntiles);
  return launch_status();
}

int vqa_gemm_bf16x6_half(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, vqa_stream_t stream) {
  clear_stale_error();
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if ((M + kHalfBM - 1) / kHalfBM * (N / kGemmBN) > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  GemmArgs g{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K, gemm_vec_ok(C, ldc, bias)};
  const int grid = static_cast<int>((M + kHalfBM - 1) / kHalfBM * (N / kGemmBN));
  gemm_bf16x6_half_kernel<<<grid, kGemmThreads, 0, static_cast<hipStream_t>(stream)>>>(g);
  return launch_status();
}

int vqa_gemm_bf16x6_tail(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, int tile, long m_split, vqa_stream_t stream) {
  clear_stale_error();
  if (tile != VQA_GEMM_TILE_256X128 && tile != VQA_GEMM_TILE_128X256) return VQA_ERR_SHAPE;
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || m_split < 0 || m_split > M) return VQA_ERR_SHAPE;
  if (m_split == M) return vqa_gemm_bf16x6_tile(A, lda, packed, bias, C, ldc, M, N, K, tile, stream);
  if (m_split == 0) return vqa_gemm_bf16x6_half(A, lda, packed, bias, C, ldc, M, N, K, stream);
  // the whole shape is checked ahead of the first launch: a refused call leaves C untouched.  Rows [m_split, M) are a
  // GEMM of their own on A + m_split * lda and C + m_split * ldc (lda % 4 == 0 keeps A on its 16-byte boundary; C's
  // alignment, and with it the vector epilogue, is worked out per part)
  if (N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  const int rc = vqa_gemm_bf16x6_tile(A, lda, packed, bias, C, ldc, m_split, N, K, tile, stream);
  if (rc != VQA_OK) return rc;
  return vqa_gemm_bf16x6_half(A + m_split * lda, lda, packed, bias, C + m_split * ldc, ldc, M - m_split, N, K, stream);
}

int vqa_gemm_bf16x6_epi(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                        int N, int K, int tile, int epilogue, float* aux, long ldaux, vqa_stream_t stream) {
  if (epilogue == VQA_GEMM_EPI_NONE) return vqa_gemm_bf16x6_tile(A, lda, packed, bias, C, ldc, M, N, K, tile, stream);
  clear_stale_error();
  if (tile != VQA_GEMM_TILE_256X128 && tile != VQA_GEMM_TILE_128X256) return VQA_ERR_SHAPE;
  if (epilogue != VQA_GEMM_EPI_GELU && epilogue != VQA_GEMM_EPI_GELU_GRAD) return VQA_ERR_SHAPE;
  if (!A || !packed || !C || (epilogue == VQA_GEMM_EPI_GELU_GRAD && !aux)) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if (aux && ldaux < N) return VQA_ERR_SHAPE;
  const bool wide = tile == VQA_GEMM_TILE_128X256 && N % kWideBN == 0;     // every other N runs the 256 x 128 tile
  const long grid = wide ? (M + kWideBM - 1) / kWideBM * (N / kWideBN) : (M + kGemmBM - 1) / kGemmBM * (N / kGemmBN);
  if (grid > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias)) || (aux && !aligned4(aux)))
    return VQA_ERR_ALIGN;
  if (aux && (aux == C || aux == A)) return VQA_ERR_SHAPE;
  if (M == 0) return VQA_OK;
  GemmEpiArgs e{{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K, gemm_vec_ok(C, ldc, bias, aux, ldaux)},
                aux, ldaux};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nwg = static_cast<int>(grid);
  if (wide) {
    if (epilogue == VQA_GEMM_EPI_GELU) gemm_bf16x6_wide_epi_kernel<VQA_GEMM_EPI_GELU><<<nwg, kGemmThreads, 0, st>>>(e);
    else gemm_bf16x6_wide_epi_kernel<VQA_GEMM_EPI_GELU_GRAD><<<nwg, kGemmThreads, 0, st>>>(e);
  } else {
    if (epilogue == VQA_GEMM_EPI_GELU) gemm_bf16x6_epi_kernel<VQA_GEMM_EPI_GELU><<<nwg, kGemmThreads, 0, st>>>(e);
    else gemm_bf16x6_epi_kernel<VQA_GEMM_EPI_GELU_GRAD><<<nwg, kGemmThreads, 0, st>>>(e);
  }
  return launch_status();
}

int vqa_gemm_bf16x6_grouped(const float* const* A, const long* lda, const void* const* packed, const float* const* bias,
                            float* const* C, const long* ldc, float* const* aux, const long* ldaux, const long* M,
                            int n_groups, int N, int K, int epilogue, vqa_stream_t stream) {
  clear_stale_error();
  if (n_groups < 1 || n_groups > VQA_GEMM_MAX_GROUPS) return VQA_ERR_SHAPE;
  if (epilogue != VQA_GEMM_EPI_NONE && epilogue != VQA_GEMM_EPI_GELU && epilogue != VQA_GEMM_EPI_GELU_GRAD) return VQA_ERR_SHAPE;
  if (!A || !lda || !packed || !C || !ldc || !M || (aux && !ldaux)) return VQA_ERR_NULL;
  if (N <= 0 || K <= 0 || K % kGemmBK || N % kWideBN) return VQA_ERR_SHAPE;
  // every group is checked ahead of the launch: a refused call leaves every C untouched.  A group without rows is
  // skipped whatever its pointers are
  GemmGroupedArgs ga{};
  ga.N = N, ga.K = K, ga.vec = 1;
  long blocks = 0;
  for (int i = 0; i < n_groups; ++i) {
    if (M[i] < 0) return VQA_ERR_SHAPE;
    ga.start[i] = static_cast<int>(blocks);
    if (M[i] == 0) continue;
    const float* b = bias ? bias[i] : nullptr;
    float* x = (aux && epilogue != VQA_GEMM_EPI_NONE) ? aux[i] : nullptr;        // no epilogue: aux, ldaux ignored
    const long ldx = x ? ldaux[i] : 0;
    if (!A[i] || !packed[i] || !C[i] || (epilogue == VQA_GEMM_EPI_GELU_GRAD && !x)) return VQA_ERR_NULL;
    if (lda[i] < K || lda[i] % 4 || ldc[i] < N || (x && ldx < N)) return VQA_ERR_SHAPE;
    blocks += (M[i] + kWideBM - 1) / kWideBM;
    if (blocks * (N / kWideBN) > 0x7fffffffL) return VQA_ERR_SHAPE;
    if (!aligned16(A[i]) || !aligned16(packed[i]) || !aligned4(C[i]) || (b && !aligned4(b)) || (x && !aligned4(x)))
      return VQA_ERR_ALIGN;
    if (x && (x == C[i] || x == A[i])) return VQA_ERR_SHAPE;
    ga.grp[i] = GemmGroup{A[i], static_cast<const bf16x8*>(packed[i]), b, C[i], x, lda[i], ldc[i], ldx, M[i]};
    ga.vec = ga.vec && gemm_vec_ok(C[i], ldc[i], b, x, ldx);
  }
  for (int i = n_groups; i <= VQA_GEMM_MAX_GROUPS; ++i) ga.start[i] = static_cast<int>(blocks);
  if (blocks == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nwg = static_cast<int>(blocks * (N / kWideBN));
  if (epilogue == VQA_GEMM_EPI_GELU) gemm_bf16x6_grouped_kernel<VQA_GEMM_EPI_GELU><<<nwg, kGemmThreads, 0, st>>>(ga);
  else if (epilogue == VQA_GEMM_EPI_GELU_GRAD) gemm_bf16x6_grouped_kernel<VQA_GEMM_EPI_GELU_GRAD><<<nwg, kGemmThreads, 0, st>>>(ga);
  else gemm_bf16x6_grouped_kernel<VQA_GEMM_EPI_NONE><<<nwg, kGemmThreads, 0, st>>>(ga);
  return launch_status();
}

long vqa_gemm_lse_ws_floats(long M, int N) {
  if (M <= 0 || N <= 0 || N % kGemmBN) return 0;
  return (static_cast<long>(N / 64) * 2 + 1) * M;        // the pairs, then tgt
}

int vqa_gemm_bf16x6_lse(const float* A, long lda, const void* packed, const float* bias, long M, int N, int K,
                        int n_valid, const int64_t* targets, long ignore_index, float* ws, float* row_loss, float* lse,
                        int* flag, int tile, vqa_stream_t stream) {
  clear_stale_error();
  if (tile != VQA_GEMM_TILE_256X128 && tile != VQA_GEMM_TILE_128X256) return VQA_ERR_SHAPE;
  if (!A || !packed || !targets || !ws || !row_loss) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4) return VQA_ERR_SHAPE;
  if (n_valid <= 0 || n_valid > N) return VQA_ERR_SHAPE;
  const bool wide = tile == VQA_GEMM_TILE_128X256 && N % kWideBN == 0;     // every other N runs the 256 x 128 tile
  const long grid = wide ? (M + kWideBM - 1) / kWideBM * (N / kWideBN) : (M + kGemmBM - 1) / kGemmBM * (N / kGemmBN);
  if (grid > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (!aligned16(A) || !aligned16(packed) || !aligned16(ws) || (bias && !aligned4(bias)) || !aligned4(row_loss) ||
      (lse && !aligned4(lse)) || (flag && !aligned4(flag)) || (reinterpret_cast<uintptr_t>(targets) & 7u))
    return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  const int nblk = N / 64;
  f32x2* part = reinterpret_cast<f32x2*>(ws);
  float* tgt = ws + static_cast<long>(nblk) * 2 * M;
  GemmEpiArgs e{{A, static_cast<const bf16x8*>(packed), bias, nullptr, lda, 0, M, N, K, !bias || aligned16(bias)},
                nullptr, 0, targets, part, tgt, n_valid};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) gemm_bf16x6_wide_epi_kernel<VQA_GEMM_EPI_LSE><<<static_cast<int>(grid), kGemmThreads, 0, st>>>(e);
  else gemm_bf16x6_epi_kernel<VQA_GEMM_EPI_LSE><<<static_cast<int>(grid), kGemmThreads, 0, st>>>(e);
  lse_combine_kernel<<<blocks_for(static_cast<size_t>(M), kBlock), kBlock, 0, st>>>(part, tgt, targets, ignore_index, M,
                                                                                   nblk, n_valid, row_loss, lse, flag);
  return launch_status();
}

size_t vqa_gemm_small_ws_bytes(long M, int N, int ksplit) {
  if (M <= 0 || N <= 0 || N % kGemmBN || ksplit <= 1 || ksplit > kGemmMaxKSplit) return 0;
  return static_cast<size_t>(ksplit) * static_cast<size_t>(M) * N * sizeof(float);
}

int vqa_gemm_bf16x6_small(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                          int N, int K, int ksplit, void* ws, vqa_stream_t stream) {
  clear_stale_error();
  if (!A || !packed || !C) return VQA_ERR_NULL;
  if (M < 0 || N <= 0 || K <= 0 || K % kGemmBK || N % kGemmBN || lda < K || lda % 4 || ldc < N) return VQA_ERR_SHAPE;
  if (ksplit < 1 || ksplit > kGemmMaxKSplit || ksplit > K / kGemmBK) return VQA_ERR_SHAPE;
  if ((M + kSmallBM - 1) / kSmallBM * (N / kGemmBN) * ksplit > 0x7fffffffL) return VQA_ERR_SHAPE;
  if (ksplit > 1 && !ws) return VQA_ERR_NULL;
  if (!aligned16(A) || !aligned16(packed) || !aligned4(C) || (bias && !aligned4(bias))) return VQA_ERR_ALIGN;
  if (ksplit > 1 && !aligned16(ws)) return VQA_ERR_ALIGN;
  if (M == 0) return VQA_OK;
  GemmArgs g{A, static_cast<const bf16x8*>(packed), bias, C, lda, ldc, M, N, K};
  const int grid = static_cast<int>((M + kSmallBM - 1) / kSmallBM * (N / kGemmBN) * ksplit);
  gemm_bf16x6_small_kernel<<<grid, kSmallThreads, 0, static_cast<hipStream_t>(stream)>>>(g, static_cast<float*>(ws), ksplit);
  if (ksplit > 1) {
    const int vec = aligned16(C) && ldc % 4 == 0;
    gemm_splitk_combine_kernel<<<blocks_for(static_cast<size_t>(M) * (N / 4), kBlock), kBlock, 0,
                                 static_cast<hipStream_t>(stream)>>>(static_cast<const f32x4*>(ws), bias, C, ldc, M, N,
                                                                     ksplit, vec);
  }
  return launch_status();
}

}  // extern "C"
