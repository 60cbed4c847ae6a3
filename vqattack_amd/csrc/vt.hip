// Variance tuning (VMI / VNI-FGSM) kernels of the PGD loop (gfx950 / MI355X).
//
// Pure HBM streams on the tile loop of stream.hpp.  Gradient pointers travel BY VALUE in the kernel arguments and are
// indexed statically -- one instance per count, fully unrolled, no scratch.  The neighbours kernel carries the project's
// only device-side random number generator: Philox4x32-10, one block of four words per 16 bytes written, keyed from a
// device row so that a captured launch draws fresh numbers at every replay.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "stream.hpp"

namespace vqa {

constexpr int kVtMax = VQA_VT_MAX_CHUNK;

struct VtGrads {
  const float* g[kVtMax];
};

// ---- Philox4x32-10 (Salmon et al. 2011), standard constants ------------------------------------------------------
struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                          uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    // one 64-bit product per multiplier: both halves from one v_mad_u64_u32 instead of v_mul_hi_u32 + v_mul_lo_u32
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// word -> r in [-bound, bound): u = float(word >> 8) * 2^-24, u * 2 and - 1 are exact, the product with bound rounds
__host__ __device__ __forceinline__ float vt_uniform(uint32_t word, float bound) {
  const float u = static_cast<float>(word >> 8) * 5.9604644775390625e-8f;
  return (u * 2.0f - 1.0f) * bound;
}

struct VtKey {
  uint32_t k0, k1, t;
};
__device__ __forceinline__ VtKey vt_key(const uint32_t* key_dev) {   // plain loads: re-read at every (re)launch
  return VtKey{key_dev[0], key_dev[1], key_dev[2]};
}

// ---- the neighbours: out[c * copy_stride + e] = base[e] + r_{first + c}[e] ----------------------------------------
// x is read once (non-temporal); m is re-read by the momentum step that follows the model calls, so it is loaded
// plainly; NT bit1: non-temporal stores (neighbours larger than the Infinity Cache; smaller ones are re-read from it by
// the next forward).  The 16-byte index i of the tensor IS e / 4, so the four words of one Philox block are the four
// lanes of one store.
template <int C, bool NI, int NT>
struct VtNeighborsTile {
  const f32x4* x;
  const f32x4* m;
  f32x4* out;
  size_t stride4;
  uint32_t first;
  uint64_t block_offset;
  float bound, lookahead;
  VtKey key;
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
    const uint64_t j = block_offset + i;
    const Philox4 z = philox4x32_10(static_cast<uint32_t>(j), static_cast<uint32_t>(j >> 32), first + c, key.t, key.k0,
                                    key.k1);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = s.x[k] + vt_uniform(z.w[k], bound);
    st4<2, NT>(out + static_cast<size_t>(c) * stride4 + i, r);
  }
};

template <int C, bool NI, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_neighbors_vec_kernel(const f32x4* __restrict__ x,
                                                                  const f32x4* __restrict__ m, f32x4* __restrict__ out,
                                                                  size_t n4, size_t stride4, uint32_t first,
                                                                  uint64_t block_offset, float bound, float lookahead,
                                                                  const uint32_t* __restrict__ key_dev) {
  stream_tiles<U>(VtNeighborsTile<C, NI, NT>{x, m, out, stride4, first, block_offset, bound, lookahead, vt_key(key_dev)},
                  n4);
}

// scalar path: n % 4 != 0, copy_stride % 4 != 0 or a pointer that is not 16-byte aligned.  One Philox block per
// element, of which word e % 4 is used: four times the integer work, the same bits.
template <int C, bool NI>
__global__ __launch_bounds__(kBlock) void vt_neighbors_scalar_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ m,
                                                                     float* __restrict__ out, size_t n,
                                                                     size_t copy_stride, uint32_t first,
                                                                     uint64_t block_offset, float bound,
                                                                     float lookahead,
                                                                     const uint32_t* __restrict__ key_dev) {
  const VtKey key = vt_key(key_dev);
  for (size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; e < n;
       e += static_cast<size_t>(gridDim.x) * kBlock) {
    const float v = lookahead_base<NI>(x[e], NI ? m[e] : 0.0f, lookahead);
    const uint64_t j = block_offset + e / 4;
    const unsigned lane = static_cast<unsigned>(e & 3);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const Philox4 z = philox4x32_10(static_cast<uint32_t>(j), static_cast<uint32_t>(j >> 32), first + c, key.t,
                                      key.k0, key.k1);
      const uint32_t word = lane == 0 ? z.w[0] : lane == 1 ? z.w[1] : lane == 2 ? z.w[2] : z.w[3];   // no indexing
      out[static_cast<size_t>(c) * copy_stride + e] = v + vt_uniform(word, bound);
    }
  }
}

template <int C, bool NI>
static void launch_vt_neighbors_c(bool vec, size_t span_bytes, hipStream_t st, const float* x, const float* m,
                                  float* out, size_t n, size_t copy_stride, uint32_t first, uint64_t block_offset,
                                  float bound, float lookahead, const uint32_t* key_dev) {
  if (!vec) {
    vt_neighbors_scalar_kernel<C, NI><<<stream_grid(n, 1), kBlock, 0, st>>>(x, m, out, n, copy_stride, first,
                                                                           block_offset, bound, lookahead, key_dev);
    return;
  }
  constexpr int U = unroll_for(2);
  const size_t n4 = n / 4;
  dispatch_nt<false>(span_bytes, false, [&](auto nt) {
    vt_neighbors_vec_kernel<C, NI, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(m), reinterpret_cast<f32x4*>(out), n4,
        copy_stride / 4, first, block_offset, bound, lookahead, key_dev);
  });
}

// ---- the running sum of the neighbours' gradients ----------------------------------------------------------------
// acc = INIT ? g_0 : sum + g_0, then acc = acc + g_i ascending.  Gradients are read exactly once: non-temporal; the sum
// is re-read by the next accumulate or by the tune step: plain, NT bit1 for one larger than the Infinity Cache.
template <int C, bool INIT, class T>
__device__ __forceinline__ T vt_sum(const T& s, const T (&g)[C]) {
  T acc = INIT ? g[0] : s + g[0];
#pragma unroll
  for (int c = 1; c < C; ++c) acc = acc + g[c];
  return acc;
}

template <int C, bool INIT, int NT>
struct VtAccumulateTile {
  VtGrads a;
  f32x4* sum;
  struct Slot {
    f32x4 s = {}, g[C];
  };
  __device__ __forceinline__ void load(Slot& s, size_t i) const {
    if (!INIT) s.s = sum[i];
#pragma unroll
    for (int c = 0; c < C; ++c) s.g[c] = ld4_once(reinterpret_cast<const f32x4*>(a.g[c]) + i);
  }
  __device__ __forceinline__ void compute(Slot& s, bool&) const { s.s = vt_sum<C, INIT>(s.s, s.g); }
  static constexpr int kOutputs = 1;
  __device__ __forceinline__ void store(const Slot& s, size_t i, int) const { st4<2, NT>(sum + i, s.s); }
};

template <int C, bool INIT, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_accumulate_vec_kernel(VtGrads a, f32x4* sum, size_t n4) {
  stream_tiles<U>(VtAccumulateTile<C, INIT, NT>{a, sum}, n4);
}

template <int C, bool INIT>
__global__ __launch_bounds__(kBlock) void vt_accumulate_scalar_kernel(VtGrads a, float* sum, size_t n) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = a.g[c][i];
    sum[i] = vt_sum<C, INIT>(INIT ? 0.0f : sum[i], g);
  }
}

template <int C, bool INIT>
static void launch_vt_accumulate_c(bool vec, hipStream_t st, const VtGrads& a, float* sum, size_t n) {
  if (!vec) {
    vt_accumulate_scalar_kernel<C, INIT><<<stream_grid(n, 1), kBlock, 0, st>>>(a, sum, n);
    return;
  }
  constexpr int U = unroll_for(C + (INIT ? 0 : 1));
  const size_t n4 = n / 4;
  dispatch_nt<false>(n * sizeof(float), false, [&](auto nt) {
    vt_accumulate_vec_kernel<C, INIT, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        a, reinterpret_cast<f32x4*>(sum), n4);
  });
}

// ---- the tune step, alone or fused with the L-infinity update ------------------------------------------------------
// ghat = g + v (the old v), v = w * vsum - g; then out = ghat | FgmOp(x, ghat) | StepOp(x, ghat, x0).  Every element is
// read by the thread that writes it, so ghat may be g and out may be x.  g, vsum and x0 are read exactly once: always
// non-temporal; v is re-read by the next evaluation: plain.  NT bit1: non-temporal stores of out and v (results larger
// than the Infinity Cache), NT bit2: non-temporal loads of x (never for an in-place update).
// One element (or 16-byte piece): ghat and the new v.
template <class T>
__device__ __forceinline__ void vt_tune(float w, const T& g, const T& vsum, T& v, T& ghat) {
  ghat = g + v;
  v = w * vsum - g;
}

template <int FORM, int NT>
struct VtTuneTile {
  const f32x4* x;
  const f32x4* g;
  const f32x4* vsum;
  f32x4* v;
  const f32x4* x0;
  f32x4* out;
  float w;
  StepParams p;
  struct Slot {
    f32x4 x = {}, g, vsum, v, x0 = {}, r;
  };
  __device__ __forceinline__ void load(Slot& s, size_t i) const {
    if (FORM != kNoImage) s.x = ld4<4, NT>(x + i);
    s.g = ld4_once(g + i);
    s.vsum = ld4_once(vsum + i);
    s.v = v[i];
    if (FORM == kStep) s.x0 = ld4_once(x0 + i);
  }
  __device__ __forceinline__ void compute(Slot& s, bool& bad) const {
    vt_tune(w, s.g, s.vsum, s.v, s.r);
    s.r = image<FORM>(p, s.x, s.r, s.x0, bad);
  }
  static constexpr int kOutputs = 2;
  __device__ __forceinline__ void store(const Slot& s, size_t i, int o) const {
    if (o == 0) st4<2, NT>(v + i, s.v);
    else st4<2, NT>(out + i, s.r);
  }
};

template <int FORM, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_tune_vec_kernel(const f32x4* x,   // may alias out
                                                             const f32x4* g,   // may alias out in the tune form
                                                             const f32x4* __restrict__ vsum, f32x4* v,
                                                             const f32x4* __restrict__ x0, f32x4* out, size_t n4,
                                                             float w, StepParams p, int* __restrict__ flag) {
  const bool bad = stream_tiles<U>(VtTuneTile<FORM, NT>{x, g, vsum, v, x0, out, w, p}, n4);
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void vt_tune_scalar_kernel(const float* x, const float* g,
                                                                const float* __restrict__ vsum, float* v,
                                                                const float* __restrict__ x0, float* out, size_t n,
                                                                float w, StepParams p, int* __restrict__ flag) {
  constexpr bool kImage = FORM != kNoImage;
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float vi = v[i], gh;
    vt_tune(w, g[i], vsum[i], vi, gh);
    v[i] = vi;
    out[i] = image<FORM>(p, kImage ? x[i] : 0.0f, gh, FORM == kStep ? x0[i] : 0.0f, bad);
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM>
static int launch_vt_tune(const float* x, const float* g, const float* vsum, float* v, const float* x0, float* out,
                          size_t n, float w, const StepParams& p, int* flag, vqa_stream_t stream) {
  constexpr bool kImage = FORM != kNoImage;
  if (!g || !vsum || !v || !out || (kImage && !x) || (FORM == kStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  if (n) {
    if (ranges_overlap(g, nb, vsum, nb) || ranges_overlap(g, nb, v, nb) || ranges_overlap(vsum, nb, v, nb)) return VQA_ERR_SHAPE;
    if (ranges_overlap(out, nb, vsum, nb) || ranges_overlap(out, nb, v, nb)) return VQA_ERR_SHAPE;
    if (kImage ? ranges_overlap(out, nb, g, nb) : (out != g && ranges_overlap(out, nb, g, nb))) return VQA_ERR_SHAPE;
    if (FORM == kStep && ranges_overlap(x0, nb, out, nb)) return VQA_ERR_SHAPE;
    if (FORM == kStep && ranges_overlap(x0, nb, v, nb)) return VQA_ERR_SHAPE;
    if (kImage && x != out && ranges_overlap(x, nb, out, nb)) return VQA_ERR_SHAPE;   // exactly in place, or apart
    if (kImage && ranges_overlap(x, nb, v, nb)) return VQA_ERR_SHAPE;
  }
  if (!aligned4(g) || !aligned4(vsum) || !aligned4(v) || !aligned4(out) || (kImage && !aligned4(x)) ||
      (FORM == kStep && !aligned4(x0)))
    return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  const bool vec = (n % 4 == 0) && aligned16(g) && aligned16(vsum) && aligned16(v) && aligned16(out) &&
                   (!kImage || aligned16(x)) && (FORM != kStep || aligned16(x0));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!vec) {
    vt_tune_scalar_kernel<FORM><<<stream_grid(n, 1), kBlock, 0, st>>>(x, g, vsum, v, x0, out, n, w, p, flag);
    return launch_status();
  }
  constexpr int U = unroll_for(3 + (kImage ? 1 : 0) + (FORM == kStep ? 1 : 0));   // g, vsum, v and the image's streams
  const size_t n4 = n / 4;
  dispatch_nt<kImage>(nb, x == out, [&](auto nt) {
    vt_tune_vec_kernel<FORM, U, decltype(nt)::value><<<stream_grid(n4, U), kBlock, 0, st>>>(
        reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(g), reinterpret_cast<const f32x4*>(vsum),
        reinterpret_cast<f32x4*>(v), reinterpret_cast<const f32x4*>(x0), reinterpret_cast<f32x4*>(out), n4, w, p, flag);
  });
  return launch_status();
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_vt_max_chunk(void) { return VQA_VT_MAX_CHUNK; }

int vqa_vt_neighbors(const float* x, const float* m, float* out, size_t n, size_t copy_stride, int count, int first,
                     unsigned long long block_offset, float bound, float lookahead, const unsigned* key_dev,
                     vqa_stream_t stream) {
  clear_stale_error();
  if (!x || !out || !key_dev) return VQA_ERR_NULL;
  if (count < 1 || count > kVtMax || first < 0) return VQA_ERR_SHAPE;
  CopiesSpan span;
  if (const int err = check_copies(span, x, m, key_dev, 3 * sizeof(unsigned), out, n, n, copy_stride, count)) return err;
  if (n == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t f = static_cast<uint32_t>(first);
  const uint64_t off = static_cast<uint64_t>(block_offset);
  dispatch_count<kVtMax>(count, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (m) launch_vt_neighbors_c<C, true>(span.vec, span.bytes, st, x, m, out, n, copy_stride, f, off, bound, lookahead, key_dev);
    else launch_vt_neighbors_c<C, false>(span.vec, span.bytes, st, x, nullptr, out, n, copy_stride, f, off, bound, lookahead, key_dev);
  });
  return launch_status();
}

int vqa_vt_accumulate(const float* const* grads_host, int count, float* sum, size_t n, int init, vqa_stream_t stream) {
  clear_stale_error();
  if (!grads_host || !sum) return VQA_ERR_NULL;
  VtGrads a;
  uintptr_t low = reinterpret_cast<uintptr_t>(sum);
  if (const int err = pack_streams(a.g, low, grads_host, count, sum, n * sizeof(float))) return err;   // sum may alias no gradient
  if (low & 3u) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  const bool vec = (n % 4 == 0) && (low & 15u) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_count<kVtMax>(count, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (init) launch_vt_accumulate_c<C, true>(vec, st, a, sum, n);
    else launch_vt_accumulate_c<C, false>(vec, st, a, sum, n);
  });
  return launch_status();
}

int vqa_vt_tune(const float* g, const float* vsum, float* v, float* ghat, size_t n, float w, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_vt_tune<kNoImage>(nullptr, g, vsum, v, nullptr, ghat, n, w, p, nullptr, stream);
}

int vqa_linf_vt_step(const float* x, const float* g, const float* vsum, float* v, const float* x0, float* out, size_t n,
                     float w, float eps_iter, float eps, float cmin, float cmax, unsigned mode, int* flag,
                     vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_vt_tune<kStep>(x, g, vsum, v, x0, out, n, w, p, flag, stream);
  return launch_vt_tune<kFgm>(x, g, vsum, v, nullptr, out, n, w, p, flag, stream);
}

}  // extern "C"
