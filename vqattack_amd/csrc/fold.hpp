// The weighted fold of a list of gradient streams, alone or with the L-infinity update behind it: si.hip's combine
// (SEED = false: the fold starts from its first product) and admix.hip's running sum (SEED = true: it starts from a
// stream `acc`).  One element function, one vector kernel, one scalar kernel and one launcher; each of the two files
// instantiates its own SEED value only, so a kernel's name says which file it is compiled from.
//
// The gradient streams are separate tensors (autograd hands back one per copy): their pointers and weights travel BY
// VALUE in the kernel arguments and are indexed statically -- one instance per copy count, fully unrolled, no scratch.
// Read streams: copies (+ 1 seeded) alone, copies + 2 (+ 1) with the step.  Unseeded: unroll_for(copies) slots; seeded:
// one slot (unroll_for(copies + 3) = 1).
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#pragma once
#include "stream.hpp"

namespace vqa {

constexpr int kFoldMax = VQA_SI_MAX_COPIES;

struct Scales {
  float s[kFoldMax];
};
struct GradList {
  const float* g[kFoldMax];
  float w[kFoldMax];
};

// One element (or 16-byte piece) of the fold: acc = [seed +] w_0 * g_0, then acc = acc + w_i * g_i in ascending i.
// Unseeded, the accumulator starts from the first product (not from +0), so copies = 1, w = {1} is the exact identity,
// -0 and NaN payloads included.  Then out = acc | FgmOp(x, acc) | StepOp(x, acc, x0).
template <bool SEED, int FORM, int C, class T>
__device__ __forceinline__ T grad_fold(const GradList& a, const StepParams& p, const T& x, const T& seed,
                                       const T (&g)[C], const T& x0, bool& bad) {
  T acc = SEED ? seed : a.w[0] * g[0];
#pragma unroll
  for (int c = SEED ? 0 : 1; c < C; ++c) acc = acc + a.w[c] * g[c];
  return image<FORM>(p, x, acc, x0, bad);
}

// NT bit1: non-temporal stores of `out` (a result larger than the Infinity Cache), NT bit2: non-temporal loads of x
// (never for an in-place update).  Gradients and x0 are read exactly once: always non-temporal.  The seed: FORM kNoImage
// writes the sum back to it (out == acc: the next group continues it, so it is loaded plainly); the image forms read it
// for the last time (non-temporal) and write the image alone.  SEED = false never reads `acc`.
// This kernel keeps a loop of its own, in the form of stream_tiles().  Through a tile struct -- or a device function
// shared by one __global__ wrapper per file -- the compiler reads the whole GradList at the kernel's entry and keeps
// the 8 pointers live across the loop for the partial tile, next to the loop's own advancing copies: the unseeded image
// forms with 6 to 8 copies then need more than the 96 scalar registers of 8 waves per SIMD (profiles/r26/README.md,
// profiles/r28/README.md).  Written out, each use reads the kernel arguments where it stands.  With one stream more the
// seeded 8-gradient image forms take 98 (FGM) and 100 (step) scalar registers, every other instance at most 96; the
// compiler reports 8 waves per SIMD for all of them (profiles/r27/README.md).
template <bool SEED, int FORM, int C, int U, int NT>
__global__ __launch_bounds__(kBlock) void grad_fold_vec_kernel(const f32x4* x,     // may alias out
                                                               const f32x4* acc,   // SEED, kNoImage: is out
                                                               const f32x4* __restrict__ x0, GradList a, f32x4* out,
                                                               size_t n4, StepParams p, int* __restrict__ flag) {
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  bool bad = false;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vx[U] = {}, v0[U] = {}, va[U] = {}, vg[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (!SEED && FORM != kNoImage) vx[u] = ld4<4, NT>(x + i);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        // A load that stands ahead of this loop comes out of the optimiser behind the last gradient's.  The unseeded fold
        // is indifferent: it needs x last.  The seeded one starts from the seed and would wait for every gradient
        // first, so its loads stand inside the loop, with g_0's (profiles/r28/README.md).
        if (SEED && c == 0) {
          if (FORM != kNoImage) vx[u] = ld4<4, NT>(x + i);
          va[u] = FORM != kNoImage ? ld4_once(acc + i) : acc[i];
        }
        vg[u][c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
      }
      if (FORM == kStep) v0[u] = ld4_once(x0 + i);
    }
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) vx[u] = grad_fold<SEED, FORM, C>(a, p, vx[u], va[u], vg[u], v0[u], bad);
    // One product per slot (a single gradient, no image): without this the compiler stores each slot as soon as its
    // product is done, `L L w1 S w1 S`; the tile's stores leave together, as everywhere else.  Any wider condition
    // changes the waits of every two-slot instance (profiles/r28/README.md).
    if (U > 1 && C == 1 && FORM == kNoImage) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) st4<2, NT>(out + base + static_cast<size_t>(u) * kBlock + threadIdx.x, vx[u]);
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 vx = {}, v0 = {}, va = {}, vg[C];
        if (FORM != kNoImage) vx = ld4<4, NT>(x + i);
        if (SEED) va = FORM != kNoImage ? ld4_once(acc + i) : acc[i];
#pragma unroll
        for (int c = 0; c < C; ++c) vg[c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
        if (FORM == kStep) v0 = ld4_once(x0 + i);
        st4<2, NT>(out + i, grad_fold<SEED, FORM, C>(a, p, vx, va, vg, v0, bad));
      }
    }
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

// scalar path: n % 4 != 0 or a pointer (a gradient included) that is not 16-byte aligned
template <bool SEED, int FORM, int C>
__global__ __launch_bounds__(kBlock) void grad_fold_scalar_kernel(const float* x, const float* acc,
                                                                  const float* __restrict__ x0, GradList a, float* out,
                                                                  size_t n, StepParams p, int* __restrict__ flag) {
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = a.g[c][i];
    out[i] = grad_fold<SEED, FORM, C>(a, p, FORM != kNoImage ? x[i] : 0.0f, SEED ? acc[i] : 0.0f, g,
                                      FORM == kStep ? x0[i] : 0.0f, bad);
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <bool SEED, int FORM, int C>
static void launch_grad_fold_c(bool vec, hipStream_t st, const float* x, const float* acc, const float* x0,
                               const GradList& a, float* out, size_t n, const StepParams& p, int* flag) {
  if (!vec) {
    grad_fold_scalar_kernel<SEED, FORM, C><<<stream_grid(n, 1), kBlock, 0, st>>>(x, acc, x0, a, out, n, p, flag);
    return;
  }
  const size_t n4 = n / 4;
  constexpr int U = SEED ? 1 : unroll_for(C);
  static_assert(!SEED || unroll_for(C + 3) == 1, "the seeded fold's stream count asks for one slot");
  dispatch_nt<FORM != kNoImage>(n * sizeof(float), x == out, [&](auto nt) {
    grad_fold_vec_kernel<SEED, FORM, C, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(acc), reinterpret_cast<const f32x4*>(x0), a,
        reinterpret_cast<f32x4*>(out), n4, p, flag);
  });
}

// `acc`: the seed (SEED only).  `out`: the fold, or the image; seeded and kNoImage it is acc itself (exactly in place).
template <bool SEED, int FORM>
static int launch_grad_fold(const float* x, const float* acc, const float* const* grads_host, const float* weights_host,
                            int copies, const float* x0, float* out, size_t n, const StepParams& p, int* flag,
                            vqa_stream_t stream) {
  constexpr bool kImage = FORM != kNoImage;
  if ((SEED && !acc) || !grads_host || !weights_host || !out || (kImage && !x) || (FORM == kStep && !x0))
    return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  GradList a;
  uintptr_t low = 0;
  if (const int err = pack_streams(a.g, low, grads_host, copies, out, nb)) return err;   // out may alias no gradient
  if (SEED && kImage && n && ranges_overlap(acc, nb, out, nb)) return VQA_ERR_SHAPE;
  if (FORM == kStep && n && ranges_overlap(x0, nb, out, nb)) return VQA_ERR_SHAPE;
  if (kImage && x != out && n && ranges_overlap(x, nb, out, nb)) return VQA_ERR_SHAPE;    // exactly in place, or apart
  low |= reinterpret_cast<uintptr_t>(out) | (SEED ? reinterpret_cast<uintptr_t>(acc) : 0) |
         (kImage ? reinterpret_cast<uintptr_t>(x) : 0) | (FORM == kStep ? reinterpret_cast<uintptr_t>(x0) : 0);
  if (low & 3u) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  for (int c = 0; c < kFoldMax; ++c) a.w[c] = c < copies ? weights_host[c] : 0.0f;
  const bool vec = (n % 4 == 0) && (low & 15u) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kFoldMax>(copies, [&](auto c) {
    launch_grad_fold_c<SEED, FORM, decltype(c)::value>(vec, st, x, acc, x0, a, out, n, p, flag);
  });
  return launch_status();
}

}  // namespace vqa
