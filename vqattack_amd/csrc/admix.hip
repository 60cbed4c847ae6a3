// Admix kernels of the PGD loop (gfx950 / MI355X): the scaled copies of one MIXED image group and the running sum of
// the groups' weighted gradients, alone or with the L-infinity update behind it.
//
// Pure HBM streams on the tile loop of stream.hpp, no LDS, no MFMA (below 0.5 flop/B).  The copies kernel deals its
// grid over the samples (grid.y): the partner index is then one scalar per workgroup and no piece needs a division.
// The gradient streams are separate tensors: their pointers and weights travel BY VALUE in the kernel arguments and are
// indexed statically, as in si.hip -- one instance per copy count, fully unrolled, no scratch.  The running sum holds
// copies + 1 read streams, the step copies + 3: unroll_for(copies + 3) = one slot.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "stream.hpp"

namespace vqa {

constexpr int kAdmixMax = VQA_SI_MAX_COPIES;

struct AdmixScales {
  float s[kAdmixMax];
};
struct AdmixGrads {
  const float* g[kAdmixMax];
  float w[kAdmixMax];
};

// ---- the copies: out[c * copy_stride + b * per + e] = s_c * ((x[b, e] [+ lookahead * m[b, e]]) + eta * x[partner[b], e])
// The sample's partner: an index outside [0, batch) never addresses memory, it stands for the sample itself.
__device__ __forceinline__ size_t admix_partner(const int* __restrict__ partner, int batch) {
  const int p = partner[blockIdx.y];
  return static_cast<size_t>(p >= 0 && p < batch ? p : static_cast<int>(blockIdx.y));
}

template <bool NI, class T>
__device__ __forceinline__ T admix_mix(const T& x, const T& m, const T& xp, float eta, float lookahead) {
  const T u = eta * xp;
  return lookahead_base<NI>(x, m, lookahead) + u;
}

// x is read twice in one launch, as itself and as somebody's partner: both loads are plain, so that the second one hits
// the Infinity Cache.  m is re-read by the momentum step that follows the model calls: plain as well.  NT bit1:
// non-temporal stores (copies larger than the Infinity Cache).  The pointers start at the sample (at its partner).
template <int C, bool NI, int NT>
struct AdmixCopiesTile {
  const f32x4* x;
  const f32x4* xp;
  const f32x4* m;
  f32x4* out;
  size_t stride4;
  AdmixScales sc;
  float eta, lookahead;
  struct Slot {
    f32x4 x, xp, m = {};
  };
  __device__ __forceinline__ void load(Slot& s, size_t i) const {
    s.x = x[i];
    s.xp = xp[i];
    if (NI) s.m = m[i];
  }
  __device__ __forceinline__ void compute(Slot& s, bool&) const { s.x = admix_mix<NI>(s.x, s.m, s.xp, eta, lookahead); }
  static constexpr int kOutputs = C;
  __device__ __forceinline__ void store(const Slot& s, size_t i, int c) const {
    st4<2, NT>(out + static_cast<size_t>(c) * stride4 + i, sc.s[c] * s.x);
  }
};

template <int C, bool NI, int U, int NT>
__global__ __launch_bounds__(kBlock) void admix_copies_vec_kernel(const f32x4* __restrict__ x,
                                                                  const f32x4* __restrict__ m,
                                                                  const int* __restrict__ partner,
                                                                  f32x4* __restrict__ out, int batch, size_t per4,
                                                                  size_t stride4, AdmixScales sc, float eta,
                                                                  float lookahead) {
  constexpr size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t off = static_cast<size_t>(blockIdx.y) * per4;
  const AdmixCopiesTile<C, NI, NT> t{x + off, x + admix_partner(partner, batch) * per4, NI ? m + off : nullptr,
                                     out + off, stride4, sc, eta, lookahead};
  stream_tiles<U>(t, static_cast<size_t>(blockIdx.x) * tile, per4, static_cast<size_t>(gridDim.x) * tile);
}

// scalar path: per % 4 != 0 (sample boundaries fall inside 16-byte groups), copy_stride % 4 != 0 or a pointer that is
// not 16-byte aligned
template <int C, bool NI>
__global__ __launch_bounds__(kBlock) void admix_copies_scalar_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ m,
                                                                     const int* __restrict__ partner,
                                                                     float* __restrict__ out, int batch, size_t per,
                                                                     size_t copy_stride, AdmixScales sc, float eta,
                                                                     float lookahead) {
  const size_t off = static_cast<size_t>(blockIdx.y) * per;
  const float* xp = x + admix_partner(partner, batch) * per;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < per;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float v = admix_mix<NI>(x[off + i], NI ? m[off + i] : 0.0f, xp[i], eta, lookahead);
#pragma unroll
    for (int c = 0; c < C; ++c) out[static_cast<size_t>(c) * copy_stride + off + i] = sc.s[c] * v;
  }
}

template <int C, bool NI>
static void launch_admix_copies_c(bool vec, size_t span_bytes, hipStream_t st, const float* x, const float* m,
                                  const int* partner, float* out, int batch, size_t per, size_t copy_stride,
                                  const AdmixScales& sc, float eta, float lookahead) {
  if (!vec) {
    dim3 grid(stream_grid(per, 1, batch), batch);
    admix_copies_scalar_kernel<C, NI><<<grid, kBlock, 0, st>>>(x, m, partner, out, batch, per, copy_stride, sc, eta,
                                                               lookahead);
    return;
  }
  constexpr int U = unroll_for(NI ? 3 : 2);
  dim3 grid(stream_grid(per / 4, U, batch), batch);
  dispatch_nt<false>(span_bytes, false, [&](auto nt) {
    admix_copies_vec_kernel<C, NI, U, decltype(nt)::value><<<grid, kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(m), partner, reinterpret_cast<f32x4*>(out),
        batch, per / 4, copy_stride / 4, sc, eta, lookahead);
  });
}

// ---- the running sum: a = acc, then a = a + w_c * g_c in ascending c; acc = a | out = FgmOp(x, a) | StepOp(x, a, x0) ---
template <int FORM, int C, class T>
__device__ __forceinline__ T admix_sum(const AdmixGrads& a, const StepParams& p, const T& x, T acc, const T (&g)[C],
                                       const T& x0, bool& bad) {
#pragma unroll
  for (int c = 0; c < C; ++c) acc = acc + a.w[c] * g[c];
  return image<FORM>(p, x, acc, x0, bad);
}

// FORM kNoImage: the sum goes back to acc (out == acc: the next group continues it, so it is loaded and stored plainly up
// to the Infinity Cache's size); the image forms read acc for the last time (non-temporal) and write the image alone.
// NT bit1: non-temporal stores of the result, NT bit2: non-temporal loads of x (never for an in-place update).
// Gradients and x0 are read exactly once: always non-temporal.  As si.hip's combine this kernel keeps a loop of its own,
// in the form of stream_tiles() with one slot: each use reads the pointers from the kernel arguments where it stands.
// With one stream more than si.hip's step the 8-gradient image forms take 98 (FGM) and 100 (step) scalar registers, every
// other instance at most 96; the compiler reports 8 waves per SIMD for all of them (profiles/r27/README.md).
template <int FORM, int C, int NT>
__global__ __launch_bounds__(kBlock) void admix_accumulate_vec_kernel(const f32x4* x,     // may alias out
                                                                      const f32x4* acc,   // kNoImage: is out
                                                                      const f32x4* __restrict__ x0, AdmixGrads a,
                                                                      f32x4* out, size_t n4, StepParams p,
                                                                      int* __restrict__ flag) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  bool bad = false;
  size_t base = static_cast<size_t>(blockIdx.x) * kBlock;
  for (; base + kBlock <= n4; base += stride) {
    const size_t i = base + threadIdx.x;
    f32x4 vx = {}, v0 = {}, va, vg[C];
    if (FORM != kNoImage) vx = ld4<4, NT>(x + i);
    va = FORM != kNoImage ? ld4_once(acc + i) : acc[i];
#pragma unroll
    for (int c = 0; c < C; ++c) vg[c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
    if (FORM == kStep) v0 = ld4_once(x0 + i);
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
    st4<2, NT>(out + i, admix_sum<FORM, C>(a, p, vx, va, vg, v0, bad));
  }
  if (base < n4) {                        // the partial tile
    const size_t i = base + threadIdx.x;
    if (i < n4) {
      f32x4 vx = {}, v0 = {}, va, vg[C];
      if (FORM != kNoImage) vx = ld4<4, NT>(x + i);
      va = FORM != kNoImage ? ld4_once(acc + i) : acc[i];
#pragma unroll
      for (int c = 0; c < C; ++c) vg[c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
      if (FORM == kStep) v0 = ld4_once(x0 + i);
      st4<2, NT>(out + i, admix_sum<FORM, C>(a, p, vx, va, vg, v0, bad));
    }
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

// scalar path: n % 4 != 0 or a pointer (a gradient included) that is not 16-byte aligned
template <int FORM, int C>
__global__ __launch_bounds__(kBlock) void admix_accumulate_scalar_kernel(const float* x, const float* acc,
                                                                         const float* __restrict__ x0, AdmixGrads a,
                                                                         float* out, size_t n, StepParams p,
                                                                         int* __restrict__ flag) {
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = a.g[c][i];
    out[i] = admix_sum<FORM, C>(a, p, FORM != kNoImage ? x[i] : 0.0f, acc[i], g, FORM == kStep ? x0[i] : 0.0f, bad);
  }
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM, int C>
static void launch_admix_accumulate_c(bool vec, hipStream_t st, const float* x, const float* acc, const float* x0,
                                      const AdmixGrads& a, float* out, size_t n, const StepParams& p, int* flag) {
  if (!vec) {
    admix_accumulate_scalar_kernel<FORM, C><<<stream_grid(n, 1), kBlock, 0, st>>>(x, acc, x0, a, out, n, p, flag);
    return;
  }
  const size_t n4 = n / 4;
  static_assert(unroll_for(C + 3) == 1, "the kernel's loop is written for one slot");
  dispatch_nt<FORM != kNoImage>(n * sizeof(float), x == out, [&](auto nt) {
    admix_accumulate_vec_kernel<FORM, C, decltype(nt)::value><<<stream_grid(n4, 1), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(acc), reinterpret_cast<const f32x4*>(x0), a,
        reinterpret_cast<f32x4*>(out), n4, p, flag);
  });
}

// `out`: acc itself for kNoImage (exactly in place), else the image.
template <int FORM>
static int launch_admix_accumulate(const float* x, const float* acc, const float* const* grads_host,
                                   const float* weights_host, int copies, const float* x0, float* out, size_t n,
                                   const StepParams& p, int* flag, vqa_stream_t stream) {
  constexpr bool kImage = FORM != kNoImage;
  if (!acc || !grads_host || !weights_host || !out || (kImage && !x) || (FORM == kStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (copies < 1 || copies > kAdmixMax) return VQA_ERR_SHAPE;
  for (int c = 0; c < copies; ++c)
    if (!grads_host[c]) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  for (int c = 0; c < copies; ++c)
    if (n && ranges_overlap(grads_host[c], nb, out, nb)) return VQA_ERR_SHAPE;          // out may alias no gradient
  if (kImage && n && ranges_overlap(acc, nb, out, nb)) return VQA_ERR_SHAPE;
  if (FORM == kStep && n && ranges_overlap(x0, nb, out, nb)) return VQA_ERR_SHAPE;
  if (kImage && x != out && n && ranges_overlap(x, nb, out, nb)) return VQA_ERR_SHAPE;  // exactly in place, or apart
  bool vec = (n % 4 == 0) && aligned16(out) && aligned16(acc) && (!kImage || aligned16(x)) &&
             (FORM != kStep || aligned16(x0));
  if (!aligned4(out) || !aligned4(acc) || (kImage && !aligned4(x)) || (FORM == kStep && !aligned4(x0)))
    return VQA_ERR_ALIGN;
  AdmixGrads a;
  for (int c = 0; c < kAdmixMax; ++c) {
    a.g[c] = c < copies ? grads_host[c] : grads_host[0];
    a.w[c] = c < copies ? weights_host[c] : 0.0f;
    if (!aligned4(a.g[c])) return VQA_ERR_ALIGN;
    vec = vec && aligned16(a.g[c]);
  }
  if (n == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kAdmixMax>(copies, [&](auto c) {
    launch_admix_accumulate_c<FORM, decltype(c)::value>(vec, st, x, acc, x0, a, out, n, p, flag);
  });
  return launch_status();
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_admix_copies(const float* x, const float* m, const int* partner, float* out, int batch, size_t per,
                     size_t copy_stride, const float* scales_host, int copies, float eta, float lookahead,
                     vqa_stream_t stream) {
  clear_stale_error();
  if (!x || !partner || !out || !scales_host) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535 || copies < 1 || copies > kAdmixMax) return VQA_ERR_SHAPE;
  const size_t n = static_cast<size_t>(batch) * per;
  if (copy_stride < n) return VQA_ERR_SHAPE;
  const size_t span = (static_cast<size_t>(copies - 1) * copy_stride + n) * sizeof(float);
  const size_t nb = n * sizeof(float);
  if (n && (ranges_overlap(x, nb, out, span) || (m && ranges_overlap(m, nb, out, span)) ||
            ranges_overlap(partner, static_cast<size_t>(batch) * sizeof(int), out, span)))
    return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || !aligned4(partner) || (m && !aligned4(m))) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  AdmixScales sc;
  for (int c = 0; c < kAdmixMax; ++c) sc.s[c] = c < copies ? scales_host[c] : 0.0f;
  const bool vec = (per % 4 == 0) && (copy_stride % 4 == 0) && aligned16(x) && aligned16(out) && (!m || aligned16(m));
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kAdmixMax>(copies, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (m) launch_admix_copies_c<C, true>(vec, span, st, x, m, partner, out, batch, per, copy_stride, sc, eta, lookahead);
    else launch_admix_copies_c<C, false>(vec, span, st, x, nullptr, partner, out, batch, per, copy_stride, sc, eta, lookahead);
  });
  return launch_status();
}

int vqa_admix_accumulate(float* acc, const float* const* grads_host, const float* weights_host, int copies, size_t n,
                         vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_admix_accumulate<kNoImage>(nullptr, acc, grads_host, weights_host, copies, nullptr, acc, n, p, nullptr,
                                           stream);
}

int vqa_linf_admix_step(const float* x, const float* acc, const float* const* grads_host, const float* weights_host,
                        int copies, const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin,
                        float cmax, unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_admix_accumulate<kStep>(x, acc, grads_host, weights_host, copies, x0, out, n, p, flag, stream);
  return launch_admix_accumulate<kFgm>(x, acc, grads_host, weights_host, copies, nullptr, out, n, p, flag, stream);
}

}  // extern "C"
