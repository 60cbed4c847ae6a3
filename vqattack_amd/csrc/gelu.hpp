// Exact GELU (torch.nn.functional.gelu, approximate='none') and its derivative on PAIRS of fp32 elements: the single
// definition behind vqa_gelu_fwd / vqa_gelu_bwd (block.hip) and the GELU epilogues of the bf16x6 GEMM (gemm.hip), which
// must give each other's bits.  erf is evaluated branch-free with packed fp32 FMAs (v_pk_fma_f32: two lanes' worth of
// polynomial per slot).  Coefficients: two minimax polynomials, erf(a) = a + a * P(a^2) below 0.9277 and
// 1 - exp(Q(|a|)) above, each below 1 ulp of error in fp32.  Pairing does not affect an element's bits.
#pragma once

namespace vqa {

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float kSqrtHalf = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;      // M_2_SQRTPI * M_SQRT1_2 * 0.5
constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk(float v) { return f32x2{v, v}; }

__device__ __forceinline__ f32x2 erf2(f32x2 a) {
  const f32x2 t = __builtin_elementwise_abs(a);
  const f32x2 s = a * a;
  // |a| > 0.9277: erf = 1 - exp(r(t))
  f32x2 r = pk_fma(pk(-1.72853470e-5f), t, pk(3.83197126e-4f));
  const f32x2 u = pk_fma(pk(-3.88396438e-3f), t, pk(2.42546219e-2f));
  r = pk_fma(r, s, u);
  r = pk_fma(r, t, pk(-1.06777877e-1f));
  r = pk_fma(r, t, pk(-6.34846687e-1f));
  r = pk_fma(r, t, pk(-1.28717512e-1f));
  r = pk_fma(r, t, -t);
  r = r * pk(kLog2e);
  f32x2 big = {1.0f - __builtin_amdgcn_exp2f(r[0]), 1.0f - __builtin_amdgcn_exp2f(r[1])};
  big = f32x2{__builtin_copysignf(big[0], a[0]), __builtin_copysignf(big[1], a[1])};
  // |a| <= 0.9277: erf = a + a * p(a^2)
  f32x2 p = pk_fma(pk(-5.96761703e-4f), s, pk(4.99119423e-3f));
  p = pk_fma(p, s, pk(-2.67681349e-2f));
  p = pk_fma(p, s, pk(1.12819925e-1f));
  p = pk_fma(p, s, pk(-3.76125336e-1f));
  p = pk_fma(p, s, pk(1.28379166e-1f));
  p = pk_fma(p, a, a);
  return f32x2{t[0] > 0.927734375f ? big[0] : p[0], t[1] > 0.927734375f ? big[1] : p[1]};
}

__device__ __forceinline__ f32x2 gelu2(f32x2 x) {            // 0.5 x (1 + erf(x / sqrt 2))
  const f32x2 e = erf2(x * pk(kSqrtHalf));
  return (pk(0.5f) * x) * (pk(1.0f) + e);
}

__device__ __forceinline__ f32x2 gelu_grad2(f32x2 x) {       // cdf + x pdf
  const f32x2 cdf = pk(0.5f) * (pk(1.0f) + erf2(x * pk(kSqrtHalf)));
  const f32x2 q = (x * x) * pk(-0.5f * kLog2e);
  const f32x2 pdf = f32x2{__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])} * pk(kInvSqrt2Pi);
  return pk_fma(x, pdf, cdf);
}

}  // namespace vqa
