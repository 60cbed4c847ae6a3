// Scale-invariant / Nesterov (SI-NI-FGSM) kernels of the PGD loop (gfx950 / MI355X).
//
// Pure HBM streams like linf.hip: 16-byte accesses, 256-thread workgroups, a grid capped at 12 workgroups per CU that
// grid-strides over block-contiguous tiles; whole tiles in a loop without a branch around any load or store (so that the
// compiler's vmcnt waits stay exact, see stream4_kernel), the buffer's one partial tile guarded apart.  The gradient
// streams are separate tensors (autograd hands back one per copy): their pointers and weights travel BY VALUE in the
// kernel arguments and are indexed statically -- one instance per copy count, fully unrolled, no scratch.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "common.hpp"

namespace vqa {

constexpr int kSiMax = VQA_SI_MAX_COPIES;
constexpr size_t kSiNtStoreBytes = 256ull << 20;   // linf.hip's Infinity-Cache rule for results
// 16-byte tiles in flight per lane and stream, chosen by register count (tools/isa_loop_mix.py --src si.hip).  The
// combine holds `copies` read streams, the step copies + 2, each with an address of its own: two tiles fit the 64
// registers that keep 8 waves per SIMD up to 3 copies, one tile beyond -- which leaves the loads in flight per lane
// (tiles x streams) about level over the copy counts.  The momentum kernels settled on two tiles by the same count
// (lnorm.hip).  The copies kernel has two read streams at most and keeps two tiles at every copy count.
constexpr int kSiUnroll = 2;
constexpr int si_unroll(int copies) { return copies <= 3 ? 2 : 1; }

struct SiScales {
  float s[kSiMax];
};
struct SiGrads {
  const float* g[kSiMax];
  float w[kSiMax];
};

// One element of the combination: acc = w_0 * g_0, then acc = acc + w_i * g_i in ascending i.  The accumulator starts
// from the first product (not from +0), so copies = 1, w = {1} is the exact identity, -0 and NaN payloads included.
template <int C>
__device__ __forceinline__ f32x4 si_combine4(const SiGrads& a, const f32x4 (&v)[C]) {
  f32x4 acc = a.w[0] * v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) acc = acc + a.w[c] * v[c];
  return acc;
}

enum SiForm { kSiCombine, kSiFgm, kSiStep };   // out = ghat | FgmOp(x, ghat) | StepOp(x, ghat, x0)

template <int FORM>
__device__ __forceinline__ float si_image(const StepParams& p, float x, float g, float x0, bool& bad) {
  if (FORM == kSiStep) return StepOp::apply(p, x, g, x0, bad);
  if (FORM == kSiFgm) return FgmOp::apply(p, x, g, 0.0f, bad);
  return g;
}

// NT bit1: non-temporal stores of `out` (a result larger than the Infinity Cache), NT bit2: non-temporal loads of x
// (never for an in-place update).  Gradients and x0 are read exactly once: always non-temporal.
template <int FORM, int C, int U, int NT>
__global__ __launch_bounds__(kBlock) void si_combine_vec_kernel(const f32x4* x,   // may alias out
                                                                const f32x4* __restrict__ x0, SiGrads a, f32x4* out,
                                                                size_t n4, StepParams p, int* __restrict__ flag) {
  constexpr bool kImage = FORM != kSiCombine;
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  bool bad = false;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vx[U], v0[U], vg[U][C], r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (kImage) vx[u] = (NT & 4) ? __builtin_nontemporal_load(&x[i]) : x[i];
#pragma unroll
      for (int c = 0; c < C; ++c) vg[u][c] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(a.g[c])[i]);
      if (FORM == kSiStep) v0[u] = __builtin_nontemporal_load(&x0[i]);
    }
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const f32x4 gh = si_combine4<C>(a, vg[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        r[u][k] = si_image<FORM>(p, kImage ? vx[u][k] : 0.0f, gh[k], FORM == kSiStep ? v0[u][k] : 0.0f, bad);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (NT & 2)
        __builtin_nontemporal_store(r[u], &out[i]);
      else
        out[i] = r[u];
    }
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 vx, v0, vg[C], r;
        if (kImage) vx = (NT & 4) ? __builtin_nontemporal_load(&x[i]) : x[i];
#pragma unroll
        for (int c = 0; c < C; ++c) vg[c] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(a.g[c])[i]);
        if (FORM == kSiStep) v0 = __builtin_nontemporal_load(&x0[i]);
        const f32x4 gh = si_combine4<C>(a, vg);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          r[k] = si_image<FORM>(p, kImage ? vx[k] : 0.0f, gh[k], FORM == kSiStep ? v0[k] : 0.0f, bad);
        if (NT & 2)
          __builtin_nontemporal_store(r, &out[i]);
        else
          out[i] = r;
      }
    }
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

// scalar path: n % 4 != 0 or a pointer (a gradient included) that is not 16-byte aligned
template <int FORM, int C>
__global__ __launch_bounds__(kBlock) void si_combine_scalar_kernel(const float* x, const float* __restrict__ x0,
                                                                   SiGrads a, float* out, size_t n, StepParams p,
                                                                   int* __restrict__ flag) {
  constexpr bool kImage = FORM != kSiCombine;
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float acc = a.w[0] * a.g[0][i];
#pragma unroll
    for (int c = 1; c < C; ++c) acc = acc + a.w[c] * a.g[c][i];
    out[i] = si_image<FORM>(p, kImage ? x[i] : 0.0f, acc, FORM == kSiStep ? x0[i] : 0.0f, bad);
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM, int C>
static void launch_si_combine_c(bool vec, int nt, hipStream_t st, const float* x, const float* x0, const SiGrads& a,
                                float* out, size_t n, const StepParams& p, int* flag) {
  if (!vec) {
    si_combine_scalar_kernel<FORM, C><<<blocks_for(n, kBlock, cu_count() * 12), kBlock, 0, st>>>(x, x0, a, out, n, p,
                                                                                                flag);
    return;
  }
  const size_t n4 = n / 4;
  constexpr int U = si_unroll(C);
  const int grid = blocks_for(n4, kBlock * U, cu_count() * 12);    // linf.hip's grid
  auto x4 = reinterpret_cast<const f32x4*>(x);
  auto z4 = reinterpret_cast<const f32x4*>(x0);
  auto o4 = reinterpret_cast<f32x4*>(out);
  // the combine form has no x stream: {0, 2}; the image forms {4, 6}, or {0, 2} in place
  if constexpr (FORM != kSiCombine) {
    if ((nt & 6) == 4) {
      si_combine_vec_kernel<FORM, C, U, 4><<<grid, kBlock, 0, st>>>(x4, z4, a, o4, n4, p, flag);
      return;
    }
    if ((nt & 6) == 6) {
      si_combine_vec_kernel<FORM, C, U, 6><<<grid, kBlock, 0, st>>>(x4, z4, a, o4, n4, p, flag);
      return;
    }
  }
  if (nt & 2) si_combine_vec_kernel<FORM, C, U, 2><<<grid, kBlock, 0, st>>>(x4, z4, a, o4, n4, p, flag);
  else si_combine_vec_kernel<FORM, C, U, 0><<<grid, kBlock, 0, st>>>(x4, z4, a, o4, n4, p, flag);
}

inline bool si_overlap(const float* a, size_t na, const float* b, size_t nb) {   // [a, a + na) meets [b, b + nb)
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

template <int FORM>
static int launch_si_combine(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                             const float* x0, float* out, size_t n, const StepParams& p, int* flag,
                             vqa_stream_t stream) {
  constexpr bool kImage = FORM != kSiCombine;
  if (!grads_host || !weights_host || !out || (kImage && !x) || (FORM == kSiStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (copies < 1 || copies > kSiMax) return VQA_ERR_SHAPE;
  for (int c = 0; c < copies; ++c)
    if (!grads_host[c]) return VQA_ERR_NULL;
  for (int c = 0; c < copies; ++c)
    if (n && si_overlap(grads_host[c], n, out, n)) return VQA_ERR_SHAPE;          // out may alias no gradient
  if (FORM == kSiStep && n && si_overlap(x0, n, out, n)) return VQA_ERR_SHAPE;
  if (kImage && x != out && n && si_overlap(x, n, out, n)) return VQA_ERR_SHAPE;  // exactly in place, or apart
  bool vec = (n % 4 == 0) && aligned16(out) && (!kImage || aligned16(x)) && (FORM != kSiStep || aligned16(x0));
  if (!aligned4(out) || (kImage && !aligned4(x)) || (FORM == kSiStep && !aligned4(x0))) return VQA_ERR_ALIGN;
  SiGrads a;
  for (int c = 0; c < kSiMax; ++c) {
    a.g[c] = c < copies ? grads_host[c] : grads_host[0];
    a.w[c] = c < copies ? weights_host[c] : 0.0f;
    if (!aligned4(a.g[c])) return VQA_ERR_ALIGN;
    vec = vec && aligned16(a.g[c]);
  }
  if (n == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int nt = kImage ? 4 : 0;
  if (n * sizeof(float) > kSiNtStoreBytes) nt |= 2;
  if (x == out) nt &= ~4;
  switch (copies) {
    case 1: launch_si_combine_c<FORM, 1>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 2: launch_si_combine_c<FORM, 2>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 3: launch_si_combine_c<FORM, 3>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 4: launch_si_combine_c<FORM, 4>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 5: launch_si_combine_c<FORM, 5>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 6: launch_si_combine_c<FORM, 6>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    case 7: launch_si_combine_c<FORM, 7>(vec, nt, st, x, x0, a, out, n, p, flag); break;
    default: launch_si_combine_c<FORM, 8>(vec, nt, st, x, x0, a, out, n, p, flag); break;
  }
  return launch_status();
}

// ---- the copies: out[c * copy_stride + e] = s_c * (x[e] [+ lookahead * m[e]]) ------------------------------------
// One launch reads x (and m) once and writes every copy.  x is read once (non-temporal); m is re-read by the momentum
// step that follows the model calls, so it is loaded plainly; NT bit1: non-temporal stores (copies larger than the
// Infinity Cache; smaller ones are re-read from it by the next forward).  VSTRIDE: copy_stride % 4 == 0.
template <bool NI>
__device__ __forceinline__ float si_base(float x, float m, float lookahead) {
  return NI ? x + lookahead * m : x;
}

template <int C, bool NI, int U, int NT>
__global__ __launch_bounds__(kBlock) void si_copies_vec_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ m,
                                                               f32x4* __restrict__ out, size_t n4, size_t stride4,
                                                               SiScales sc, float lookahead) {
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vx[U], vm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      vx[u] = __builtin_nontemporal_load(&x[i]);
      if (NI) vm[u] = m[i];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) vx[u][k] = si_base<NI>(vx[u][k], NI ? vm[u][k] : 0.0f, lookahead);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t i = static_cast<size_t>(c) * stride4 + base + static_cast<size_t>(u) * kBlock + threadIdx.x;
        const f32x4 r = sc.s[c] * vx[u];
        if (NT & 2)
          __builtin_nontemporal_store(r, &out[i]);
        else
          out[i] = r;
      }
    }
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t j = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (j < n4) {
        f32x4 v = __builtin_nontemporal_load(&x[j]);
        if (NI) {
          const f32x4 mv = m[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = si_base<true>(v[k], mv[k], lookahead);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const f32x4 r = sc.s[c] * v;
          if (NT & 2)
            __builtin_nontemporal_store(r, &out[static_cast<size_t>(c) * stride4 + j]);
          else
            out[static_cast<size_t>(c) * stride4 + j] = r;
        }
      }
    }
  }
}

template <int C, bool NI>
__global__ __launch_bounds__(kBlock) void si_copies_scalar_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ m, float* __restrict__ out,
                                                                  size_t n, size_t copy_stride, SiScales sc,
                                                                  float lookahead) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float v = si_base<NI>(x[i], NI ? m[i] : 0.0f, lookahead);
#pragma unroll
    for (int c = 0; c < C; ++c) out[static_cast<size_t>(c) * copy_stride + i] = sc.s[c] * v;
  }
}

template <int C, bool NI>
static void launch_si_copies_c(bool vec, bool nt_store, hipStream_t st, const float* x, const float* m, float* out,
                               size_t n, size_t copy_stride, const SiScales& sc, float lookahead) {
  if (!vec) {
    si_copies_scalar_kernel<C, NI><<<blocks_for(n, kBlock, cu_count() * 12), kBlock, 0, st>>>(x, m, out, n, copy_stride,
                                                                                             sc, lookahead);
    return;
  }
  const size_t n4 = n / 4;
  const int grid = blocks_for(n4, kBlock * kSiUnroll, cu_count() * 12);
  auto x4 = reinterpret_cast<const f32x4*>(x);
  auto m4 = reinterpret_cast<const f32x4*>(m);
  auto o4 = reinterpret_cast<f32x4*>(out);
  if (nt_store)
    si_copies_vec_kernel<C, NI, kSiUnroll, 2><<<grid, kBlock, 0, st>>>(x4, m4, o4, n4, copy_stride / 4, sc, lookahead);
  else
    si_copies_vec_kernel<C, NI, kSiUnroll, 0><<<grid, kBlock, 0, st>>>(x4, m4, o4, n4, copy_stride / 4, sc, lookahead);
}

template <bool NI>
static void launch_si_copies(int copies, bool vec, bool nt_store, hipStream_t st, const float* x, const float* m,
                             float* out, size_t n, size_t copy_stride, const SiScales& sc, float lookahead) {
  switch (copies) {
    case 1: launch_si_copies_c<1, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 2: launch_si_copies_c<2, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 3: launch_si_copies_c<3, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 4: launch_si_copies_c<4, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 5: launch_si_copies_c<5, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 6: launch_si_copies_c<6, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    case 7: launch_si_copies_c<7, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
    default: launch_si_copies_c<8, NI>(vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead); break;
  }
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
  const size_t span = static_cast<size_t>(copies - 1) * copy_stride + n;
  if (n && (si_overlap(x, n, out, span) || (m && si_overlap(m, n, out, span)))) return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || (m && !aligned4(m))) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  SiScales sc;
  for (int c = 0; c < kSiMax; ++c) sc.s[c] = c < copies ? scales_host[c] : 0.0f;
  const bool vec = (n % 4 == 0) && (copy_stride % 4 == 0) && aligned16(x) && aligned16(out) && (!m || aligned16(m));
  const bool nt_store = span * sizeof(float) > kSiNtStoreBytes;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m) launch_si_copies<true>(copies, vec, nt_store, st, x, m, out, n, copy_stride, sc, lookahead);
  else launch_si_copies<false>(copies, vec, nt_store, st, x, nullptr, out, n, copy_stride, sc, lookahead);
  return launch_status();
}

int vqa_si_combine(const float* const* grads_host, const float* weights_host, int copies, float* out, size_t n,
                   vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_si_combine<kSiCombine>(nullptr, grads_host, weights_host, copies, nullptr, out, n, p, nullptr, stream);
}

int vqa_linf_si_step(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                     const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_si_combine<kSiStep>(x, grads_host, weights_host, copies, x0, out, n, p, flag, stream);
  return launch_si_combine<kSiFgm>(x, grads_host, weights_host, copies, nullptr, out, n, p, flag, stream);
}

}  // extern "C"
