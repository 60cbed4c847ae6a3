// Admix kernels of the PGD loop (gfx950 / MI355X): the scaled copies of one MIXED image group and the running sum of
// the groups' weighted gradients, alone or with the L-infinity update behind it.
//
// Pure HBM streams on the tile loop of stream.hpp, no LDS, no MFMA (below 0.5 flop/B).  The copies kernel deals its
// grid over the samples (grid.y): the partner index is then one scalar per workgroup and no piece needs a division.
// The running sum and the step behind it are fold.hpp's seeded fold (grad_fold_*_kernel<true, ...>): a = acc, then
// a = a + w_c * g_c in ascending c; acc = a | out = FgmOp(x, a) | StepOp(x, a, x0).
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "fold.hpp"

namespace vqa {

constexpr int kAdmixMax = kFoldMax;

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
  Scales sc;
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
                                                                  size_t stride4, Scales sc, float eta,
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
                                                                     size_t copy_stride, Scales sc, float eta,
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
                                  const Scales& sc, float eta, float lookahead) {
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
  CopiesSpan span;   // per % 4: sample boundaries must not fall inside 16-byte pieces
  if (const int err = check_copies(span, x, m, partner, static_cast<size_t>(batch) * sizeof(int), out, n, per,
                                   copy_stride, copies))
    return err;
  if (n == 0) return VQA_OK;
  Scales sc;
  for (int c = 0; c < kAdmixMax; ++c) sc.s[c] = c < copies ? scales_host[c] : 0.0f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kAdmixMax>(copies, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (m) launch_admix_copies_c<C, true>(span.vec, span.bytes, st, x, m, partner, out, batch, per, copy_stride, sc, eta, lookahead);
    else launch_admix_copies_c<C, false>(span.vec, span.bytes, st, x, nullptr, partner, out, batch, per, copy_stride, sc, eta, lookahead);
  });
  return launch_status();
}

int vqa_admix_accumulate(float* acc, const float* const* grads_host, const float* weights_host, int copies, size_t n,
                         vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_grad_fold<true, kNoImage>(nullptr, acc, grads_host, weights_host, copies, nullptr, acc, n, p, nullptr,
                                          stream);
}

int vqa_linf_admix_step(const float* x, const float* acc, const float* const* grads_host, const float* weights_host,
                        int copies, const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin,
                        float cmax, unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_grad_fold<true, kStep>(x, acc, grads_host, weights_host, copies, x0, out, n, p, flag, stream);
  return launch_grad_fold<true, kFgm>(x, acc, grads_host, weights_host, copies, nullptr, out, n, p, flag, stream);
}

}  // extern "C"
