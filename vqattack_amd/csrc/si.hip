// Scale-invariant / Nesterov (SI-NI-FGSM) kernels of the PGD loop (gfx950 / MI355X).
//
// Pure HBM streams on the tile loop of stream.hpp.  The gradient streams are separate tensors (autograd hands back one
// per copy): their pointers and weights travel BY VALUE in the kernel arguments and are indexed statically -- one
// instance per copy count, fully unrolled, no scratch.  The combine holds `copies` read streams, the step copies + 2:
// unroll_for(copies); the copies kernel has two read streams at most.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "stream.hpp"

namespace vqa {

constexpr int kSiMax = VQA_SI_MAX_COPIES;

struct SiScales {
  float s[kSiMax];
};
struct SiGrads {
  const float* g[kSiMax];
  float w[kSiMax];
};

// One element (or 16-byte piece) of the combination: acc = w_0 * g_0, then acc = acc + w_i * g_i in ascending i.  The
// accumulator starts from the first product (not from +0), so copies = 1, w = {1} is the exact identity, -0 and NaN
// payloads included.  Then out = ghat | FgmOp(x, ghat) | StepOp(x, ghat, x0).
template <int FORM, int C, class T>
__device__ __forceinline__ T si_combine(const SiGrads& a, const StepParams& p, const T& x, const T (&g)[C], const T& x0,
                                        bool& bad) {
  T acc = a.w[0] * g[0];
#pragma unroll
  for (int c = 1; c < C; ++c) acc = acc + a.w[c] * g[c];
  return image<FORM>(p, x, acc, x0, bad);
}

// NT bit1: non-temporal stores of `out` (a result larger than the Infinity Cache), NT bit2: non-temporal loads of x
// (never for an in-place update).  Gradients and x0 are read exactly once: always non-temporal.
// This kernel keeps a loop of its own, in the form of stream_tiles().  Through a tile struct the compiler reads the whole
// SiGrads at the kernel's entry and keeps the 8 pointers live across the loop for the partial tile, next to the loop's
// own advancing copies: the image forms with 6 to 8 copies then need more than the 96 scalar registers of 8 waves per
// SIMD (profiles/r26/README.md).  Written out, each use reads the kernel arguments where it stands.
template <int FORM, int C, int U, int NT>
__global__ __launch_bounds__(kBlock) void si_combine_vec_kernel(const f32x4* x,   // may alias out
                                                                const f32x4* __restrict__ x0, SiGrads a, f32x4* out,
                                                                size_t n4, StepParams p, int* __restrict__ flag) {
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  bool bad = false;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vx[U] = {}, v0[U] = {}, vg[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (FORM != kNoImage) vx[u] = ld4<4, NT>(x + i);
#pragma unroll
      for (int c = 0; c < C; ++c) vg[u][c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
      if (FORM == kStep) v0[u] = ld4_once(x0 + i);
    }
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) vx[u] = si_combine<FORM, C>(a, p, vx[u], vg[u], v0[u], bad);
#pragma unroll
    for (int u = 0; u < U; ++u) st4<2, NT>(out + base + static_cast<size_t>(u) * kBlock + threadIdx.x, vx[u]);
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 vx = {}, v0 = {}, vg[C];
        if (FORM != kNoImage) vx = ld4<4, NT>(x + i);
#pragma unroll
        for (int c = 0; c < C; ++c) vg[c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
        if (FORM == kStep) v0 = ld4_once(x0 + i);
        st4<2, NT>(out + i, si_combine<FORM, C>(a, p, vx, vg, v0, bad));
      }
    }
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

// scalar path: n % 4 != 0 or a pointer (a gradient included) that is not 16-byte aligned
template <int FORM, int C>
__global__ __launch_bounds__(kBlock) void si_combine_scalar_kernel(const float* x, const float* __restrict__ x0,
                                                                   SiGrads a, float* out, size_t n, StepParams p,
                                                                   int* __restrict__ flag) {
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = a.g[c][i];
    out[i] = si_combine<FORM, C>(a, p, FORM != kNoImage ? x[i] : 0.0f, g, FORM == kStep ? x0[i] : 0.0f, bad);
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM, int C>
static void launch_si_combine_c(bool vec, hipStream_t st, const float* x, const float* x0, const SiGrads& a, float* out,
                                size_t n, const StepParams& p, int* flag) {
  if (!vec) {
    si_combine_scalar_kernel<FORM, C><<<stream_grid(n, 1), kBlock, 0, st>>>(x, x0, a, out, n, p, flag);
    return;
  }
  const size_t n4 = n / 4;
  constexpr int U = unroll_for(C);
  dispatch_nt<FORM != kNoImage>(n * sizeof(float), x == out, [&](auto nt) {
    si_combine_vec_kernel<FORM, C, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(x0), a, reinterpret_cast<f32x4*>(out), n4, p,
        flag);
  });
}

template <int FORM>
static int launch_si_combine(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                             const float* x0, float* out, size_t n, const StepParams& p, int* flag,
                             vqa_stream_t stream) {
  constexpr bool kImage = FORM != kNoImage;
  if (!grads_host || !weights_host || !out || (kImage && !x) || (FORM == kStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (copies < 1 || copies > kSiMax) return VQA_ERR_SHAPE;
  for (int c = 0; c < copies; ++c)
    if (!grads_host[c]) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  for (int c = 0; c < copies; ++c)
    if (n && ranges_overlap(grads_host[c], nb, out, nb)) return VQA_ERR_SHAPE;          // out may alias no gradient
  if (FORM == kStep && n && ranges_overlap(x0, nb, out, nb)) return VQA_ERR_SHAPE;
  if (kImage && x != out && n && ranges_overlap(x, nb, out, nb)) return VQA_ERR_SHAPE;  // exactly in place, or apart
  bool vec = (n % 4 == 0) && aligned16(out) && (!kImage || aligned16(x)) && (FORM != kStep || aligned16(x0));
  if (!aligned4(out) || (kImage && !aligned4(x)) || (FORM == kStep && !aligned4(x0))) return VQA_ERR_ALIGN;
  SiGrads a;
  for (int c = 0; c < kSiMax; ++c) {
    a.g[c] = c < copies ? grads_host[c] : grads_host[0];
    a.w[c] = c < copies ? weights_host[c] : 0.0f;
    if (!aligned4(a.g[c])) return VQA_ERR_ALIGN;
    vec = vec && aligned16(a.g[c]);
  }
  if (n == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kSiMax>(copies, [&](auto c) {
    launch_si_combine_c<FORM, decltype(c)::value>(vec, st, x, x0, a, out, n, p, flag);
  });
  return launch_status();
}

// ---- the copies: out[c * copy_stride + e] = s_c * (x[e] [+ lookahead * m[e]]) ------------------------------------
// One launch reads x (and m) once and writes every copy.  x is read once (non-temporal); m is re-read by the momentum
// step that follows the model calls, so it is loaded plainly; NT bit1: non-temporal stores (copies larger than the
// Infinity Cache; smaller ones are re-read from it by the next forward).  The vector kernel needs copy_stride % 4 == 0.
template <int C, bool NI, int NT>
struct SiCopiesTile {
  const f32x4* x;
  const f32x4* m;
  f32x4* out;
  size_t stride4;
  SiScales sc;
  float lookahead;
  struct Slot {
    f32x4 x, m = {};
  };
  __device__ __forceinline__ void load(Slot& s, size_t i) const {
    s.x = ld4_once(x + i);
    if (NI) s.m = m[i];
  }
  __device__ __forceinline__ void compute(Slot& s, bool&) const { s.x = lookahead_base<NI>(s.x, s.m, lookahead); }
  static constexpr int kOutputs = C;
  __device__ __forceinline__ void store(const Slot& s, size_t i, int c) const {
    st4<2, NT>(out + static_cast<size_t>(c) * stride4 + i, sc.s[c] * s.x);
  }
};

template <int C, bool NI, int U, int NT>
__global__ __launch_bounds__(kBlock) void si_copies_vec_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ m,
                                                               f32x4* __restrict__ out, size_t n4, size_t stride4,
                                                               SiScales sc, float lookahead) {
  stream_tiles<U>(SiCopiesTile<C, NI, NT>{x, m, out, stride4, sc, lookahead}, n4);
}

template <int C, bool NI>
__global__ __launch_bounds__(kBlock) void si_copies_scalar_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ m, float* __restrict__ out,
                                                                  size_t n, size_t copy_stride, SiScales sc,
                                                                  float lookahead) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float v = lookahead_base<NI>(x[i], NI ? m[i] : 0.0f, lookahead);
#pragma unroll
    for (int c = 0; c < C; ++c) out[static_cast<size_t>(c) * copy_stride + i] = sc.s[c] * v;
  }
}

template <int C, bool NI>
static void launch_si_copies_c(bool vec, size_t span_bytes, hipStream_t st, const float* x, const float* m, float* out,
                               size_t n, size_t copy_stride, const SiScales& sc, float lookahead) {
  if (!vec) {
    si_copies_scalar_kernel<C, NI><<<stream_grid(n, 1), kBlock, 0, st>>>(x, m, out, n, copy_stride, sc, lookahead);
    return;
  }
  const size_t n4 = n / 4;
  constexpr int U = unroll_for(2);
  dispatch_nt<false>(span_bytes, false, [&](auto nt) {
    si_copies_vec_kernel<C, NI, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(m), reinterpret_cast<f32x4*>(out), n4,
        copy_stride / 4, sc, lookahead);
  });
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_si_max_copies(void) { return VQA_SI_MAX_COPIES; }

int vqa_si_copies(const float* x, const float* m, float* out, size_t n, size_t copy_stride, const float* scales_host,
                  int copies, float lookahead, vqa_stream_t stream) {
  clear_stale_error();
  if (!x || !out || !scales_host) return VQA_ERR_NULL;
  if (copies < 1 || copies > kSiMax || copy_stride < n) return VQA_ERR_SHAPE;
  const size_t span = (static_cast<size_t>(copies - 1) * copy_stride + n) * sizeof(float);
  const size_t nb = n * sizeof(float);
  if (n && (ranges_overlap(x, nb, out, span) || (m && ranges_overlap(m, nb, out, span)))) return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || (m && !aligned4(m))) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  SiScales sc;
  for (int c = 0; c < kSiMax; ++c) sc.s[c] = c < copies ? scales_host[c] : 0.0f;
  const bool vec = (n % 4 == 0) && (copy_stride % 4 == 0) && aligned16(x) && aligned16(out) && (!m || aligned16(m));
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kSiMax>(copies, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (m) launch_si_copies_c<C, true>(vec, span, st, x, m, out, n, copy_stride, sc, lookahead);
    else launch_si_copies_c<C, false>(vec, span, st, x, nullptr, out, n, copy_stride, sc, lookahead);
  });
  return launch_status();
}

int vqa_si_combine(const float* const* grads_host, const float* weights_host, int copies, float* out, size_t n,
                   vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_si_combine<kNoImage>(nullptr, grads_host, weights_host, copies, nullptr, out, n, p, nullptr, stream);
}

int vqa_linf_si_step(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                     const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_si_combine<kStep>(x, grads_host, weights_host, copies, x0, out, n, p, flag, stream);
  return launch_si_combine<kFgm>(x, grads_host, weights_host, copies, nullptr, out, n, p, flag, stream);
}

}  // extern "C"
