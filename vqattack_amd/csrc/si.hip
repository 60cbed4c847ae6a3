// Scale-invariant / Nesterov (SI-NI-FGSM) kernels of the PGD loop (gfx950 / MI355X).
//
// Pure HBM streams on the tile loop of stream.hpp.  The combine and the step behind it are fold.hpp's unseeded fold
// (grad_fold_*_kernel<false, ...>); the copies kernel, here, has two read streams at most.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "fold.hpp"

namespace vqa {

constexpr int kSiMax = kFoldMax;

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
  Scales sc;
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
                                                               Scales sc, float lookahead) {
  stream_tiles<U>(SiCopiesTile<C, NI, NT>{x, m, out, stride4, sc, lookahead}, n4);
}

template <int C, bool NI>
__global__ __launch_bounds__(kBlock) void si_copies_scalar_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ m, float* __restrict__ out,
                                                                  size_t n, size_t copy_stride, Scales sc,
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
                               size_t n, size_t copy_stride, const Scales& sc, float lookahead) {
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
  if (copies < 1 || copies > kSiMax) return VQA_ERR_SHAPE;
  CopiesSpan span;
  if (const int err = check_copies(span, x, m, nullptr, 0, out, n, n, copy_stride, copies)) return err;
  if (n == 0) return VQA_OK;
  Scales sc;
  for (int c = 0; c < kSiMax; ++c) sc.s[c] = c < copies ? scales_host[c] : 0.0f;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kSiMax>(copies, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (m) launch_si_copies_c<C, true>(span.vec, span.bytes, st, x, m, out, n, copy_stride, sc, lookahead);
    else launch_si_copies_c<C, false>(span.vec, span.bytes, st, x, nullptr, out, n, copy_stride, sc, lookahead);
  });
  return launch_status();
}

int vqa_si_combine(const float* const* grads_host, const float* weights_host, int copies, float* out, size_t n,
                   vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_grad_fold<false, kNoImage>(nullptr, nullptr, grads_host, weights_host, copies, nullptr, out, n, p,
                                           nullptr, stream);
}

int vqa_linf_si_step(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                     const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_grad_fold<false, kStep>(x, nullptr, grads_host, weights_host, copies, x0, out, n, p, flag, stream);
  return launch_grad_fold<false, kFgm>(x, nullptr, grads_host, weights_host, copies, nullptr, out, n, p, flag, stream);
}

}  // extern "C"
