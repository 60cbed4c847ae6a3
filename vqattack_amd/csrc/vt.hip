// Variance tuning (VMI / VNI-FGSM) kernels of the PGD loop (gfx950 / MI355X).
//
// Pure HBM streams like si.hip / linf.hip: 16-byte accesses, 256-thread workgroups, a grid capped at 12 workgroups per
// CU that grid-strides over block-contiguous tiles; whole tiles in a loop without a branch around any load or store (so
// that the compiler's vmcnt waits stay exact), the buffer's one partial tile guarded apart.  Gradient pointers travel BY
// VALUE in the kernel arguments and are indexed statically -- one instance per count, fully unrolled, no scratch.  The
// neighbours kernel carries the project's only device-side random number generator: Philox4x32-10, one block of four
// words per 16 bytes written, keyed from a device row so that a captured launch draws fresh numbers at every replay.
// Arithmetic per include/vqattack_hip.h: fp32, one rounding per operation, -ffp-contract=off.
#include "common.hpp"

namespace vqa {

constexpr int kVtMax = VQA_VT_MAX_CHUNK;
constexpr size_t kVtNtStoreBytes = 256ull << 20;   // linf.hip's Infinity-Cache rule for results
// 16-byte tiles in flight per lane and stream, by si.hip's register count: two up to 3 read streams, one beyond.
constexpr int vt_unroll(int streams) { return streams <= 3 ? 2 : 1; }

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

template <bool NI>
__device__ __forceinline__ float vt_base(float x, float m, float lookahead) {
  return NI ? x + lookahead * m : x;
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
template <int C, bool NI, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_neighbors_vec_kernel(const f32x4* __restrict__ x,
                                                                  const f32x4* __restrict__ m, f32x4* __restrict__ out,
                                                                  size_t n4, size_t stride4, uint32_t first,
                                                                  uint64_t block_offset, float bound, float lookahead,
                                                                  const uint32_t* __restrict__ key_dev) {
  const VtKey key = vt_key(key_dev);
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
      for (int k = 0; k < 4; ++k) vx[u][k] = vt_base<NI>(vx[u][k], NI ? vm[u][k] : 0.0f, lookahead);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
        const uint64_t j = block_offset + i;
        const Philox4 z = philox4x32_10(static_cast<uint32_t>(j), static_cast<uint32_t>(j >> 32), first + c, key.t,
                                        key.k0, key.k1);
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = vx[u][k] + vt_uniform(z.w[k], bound);
        const size_t o = static_cast<size_t>(c) * stride4 + i;
        if (NT & 2)
          __builtin_nontemporal_store(r, &out[o]);
        else
          out[o] = r;
      }
    }
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 v = __builtin_nontemporal_load(&x[i]);
        if (NI) {
          const f32x4 mv = m[i];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = vt_base<true>(v[k], mv[k], lookahead);
        }
        const uint64_t j = block_offset + i;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const Philox4 z = philox4x32_10(static_cast<uint32_t>(j), static_cast<uint32_t>(j >> 32), first + c, key.t,
                                          key.k0, key.k1);
          f32x4 r;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = v[k] + vt_uniform(z.w[k], bound);
          const size_t o = static_cast<size_t>(c) * stride4 + i;
          if (NT & 2)
            __builtin_nontemporal_store(r, &out[o]);
          else
            out[o] = r;
        }
      }
    }
  }
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
    const float v = vt_base<NI>(x[e], NI ? m[e] : 0.0f, lookahead);
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
static void launch_vt_neighbors_c(bool vec, bool nt_store, hipStream_t st, const float* x, const float* m, float* out,
                                  size_t n, size_t copy_stride, uint32_t first, uint64_t block_offset, float bound,
                                  float lookahead, const uint32_t* key_dev) {
  if (!vec) {
    vt_neighbors_scalar_kernel<C, NI><<<blocks_for(n, kBlock, cu_count() * 12), kBlock, 0, st>>>(
        x, m, out, n, copy_stride, first, block_offset, bound, lookahead, key_dev);
    return;
  }
  constexpr int U = 2;
  const size_t n4 = n / 4;
  const int grid = blocks_for(n4, kBlock * U, cu_count() * 12);
  auto x4 = reinterpret_cast<const f32x4*>(x);
  auto m4 = reinterpret_cast<const f32x4*>(m);
  auto o4 = reinterpret_cast<f32x4*>(out);
  if (nt_store)
    vt_neighbors_vec_kernel<C, NI, U, 2><<<grid, kBlock, 0, st>>>(x4, m4, o4, n4, copy_stride / 4, first, block_offset,
                                                                  bound, lookahead, key_dev);
  else
    vt_neighbors_vec_kernel<C, NI, U, 0><<<grid, kBlock, 0, st>>>(x4, m4, o4, n4, copy_stride / 4, first, block_offset,
                                                                  bound, lookahead, key_dev);
}

template <bool NI>
static void launch_vt_neighbors(int count, bool vec, bool nt_store, hipStream_t st, const float* x, const float* m,
                                float* out, size_t n, size_t copy_stride, uint32_t first, uint64_t block_offset,
                                float bound, float lookahead, const uint32_t* key_dev) {
#define VQA_VT_CASE(C) \
  case C: launch_vt_neighbors_c<C, NI>(vec, nt_store, st, x, m, out, n, copy_stride, first, block_offset, bound, \
                                        lookahead, key_dev); break;
  switch (count) {
    VQA_VT_CASE(1) VQA_VT_CASE(2) VQA_VT_CASE(3) VQA_VT_CASE(4) VQA_VT_CASE(5) VQA_VT_CASE(6) VQA_VT_CASE(7)
    default: launch_vt_neighbors_c<8, NI>(vec, nt_store, st, x, m, out, n, copy_stride, first, block_offset, bound,
                                          lookahead, key_dev); break;
  }
#undef VQA_VT_CASE
}

// ---- the running sum of the neighbours' gradients ----------------------------------------------------------------
// acc = INIT ? g_0 : sum + g_0, then acc = acc + g_i ascending.  Gradients are read exactly once: non-temporal; the sum
// is re-read by the next accumulate or by the tune step: plain, NT bit1 for one larger than the Infinity Cache.
template <int C, bool INIT>
__device__ __forceinline__ f32x4 vt_sum4(const f32x4& s, const f32x4 (&v)[C]) {
  f32x4 acc = INIT ? v[0] : s + v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) acc = acc + v[c];
  return acc;
}

template <int C, bool INIT, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_accumulate_vec_kernel(VtGrads a, f32x4* sum, size_t n4) {
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vs[U] = {}, vg[U][C], r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (!INIT) vs[u] = sum[i];
#pragma unroll
      for (int c = 0; c < C; ++c) vg[u][c] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(a.g[c])[i]);
    }
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = vt_sum4<C, INIT>(vs[u], vg[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (NT & 2)
        __builtin_nontemporal_store(r[u], &sum[i]);
      else
        sum[i] = r[u];
    }
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 vs = {}, vg[C];
        if (!INIT) vs = sum[i];
#pragma unroll
        for (int c = 0; c < C; ++c) vg[c] = __builtin_nontemporal_load(&reinterpret_cast<const f32x4*>(a.g[c])[i]);
        const f32x4 r = vt_sum4<C, INIT>(vs, vg);
        if (NT & 2)
          __builtin_nontemporal_store(r, &sum[i]);
        else
          sum[i] = r;
      }
    }
  }
}

template <int C, bool INIT>
__global__ __launch_bounds__(kBlock) void vt_accumulate_scalar_kernel(VtGrads a, float* sum, size_t n) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    float acc = INIT ? a.g[0][i] : sum[i] + a.g[0][i];
#pragma unroll
    for (int c = 1; c < C; ++c) acc = acc + a.g[c][i];
    sum[i] = acc;
  }
}

template <int C, bool INIT>
static void launch_vt_accumulate_c(bool vec, bool nt_store, hipStream_t st, const VtGrads& a, float* sum, size_t n) {
  if (!vec) {
    vt_accumulate_scalar_kernel<C, INIT><<<blocks_for(n, kBlock, cu_count() * 12), kBlock, 0, st>>>(a, sum, n);
    return;
  }
  constexpr int U = vt_unroll(C + (INIT ? 0 : 1));
  const size_t n4 = n / 4;
  const int grid = blocks_for(n4, kBlock * U, cu_count() * 12);
  auto s4 = reinterpret_cast<f32x4*>(sum);
  if (nt_store) vt_accumulate_vec_kernel<C, INIT, U, 2><<<grid, kBlock, 0, st>>>(a, s4, n4);
  else vt_accumulate_vec_kernel<C, INIT, U, 0><<<grid, kBlock, 0, st>>>(a, s4, n4);
}

template <bool INIT>
static void launch_vt_accumulate(int count, bool vec, bool nt_store, hipStream_t st, const VtGrads& a, float* sum,
                                 size_t n) {
  switch (count) {
    case 1: launch_vt_accumulate_c<1, INIT>(vec, nt_store, st, a, sum, n); break;
    case 2: launch_vt_accumulate_c<2, INIT>(vec, nt_store, st, a, sum, n); break;
    case 3: launch_vt_accumulate_c<3, INIT>(vec, nt_store, st, a, sum, n); break;
    case 4: launch_vt_accumulate_c<4, INIT>(vec, nt_store, st, a, sum, n); break;
    case 5: launch_vt_accumulate_c<5, INIT>(vec, nt_store, st, a, sum, n); break;
    case 6: launch_vt_accumulate_c<6, INIT>(vec, nt_store, st, a, sum, n); break;
    case 7: launch_vt_accumulate_c<7, INIT>(vec, nt_store, st, a, sum, n); break;
    default: launch_vt_accumulate_c<8, INIT>(vec, nt_store, st, a, sum, n); break;
  }
}

// ---- the tune step, alone or fused with the L-infinity update ------------------------------------------------------
// ghat = g + v (the old v), v = w * vsum - g; then out = ghat | FgmOp(x, ghat) | StepOp(x, ghat, x0).  Every element is
// read by the thread that writes it, so ghat may be g and out may be x.  g, vsum and x0 are read exactly once: always
// non-temporal; v is re-read by the next evaluation: plain.  NT bit1: non-temporal stores of out and v (results larger
// than the Infinity Cache), NT bit2: non-temporal loads of x (never for an in-place update).
enum VtForm { kVtTune, kVtFgm, kVtStep };

template <int FORM>
__device__ __forceinline__ float vt_image(const StepParams& p, float x, float g, float x0, bool& bad) {
  if (FORM == kVtStep) return StepOp::apply(p, x, g, x0, bad);
  if (FORM == kVtFgm) return FgmOp::apply(p, x, g, 0.0f, bad);
  return g;
}

template <int FORM, int U, int NT>
__global__ __launch_bounds__(kBlock) void vt_tune_vec_kernel(const f32x4* x,   // may alias out
                                                             const f32x4* g,   // may alias out in the tune form
                                                             const f32x4* __restrict__ vsum, f32x4* v,
                                                             const f32x4* __restrict__ x0, f32x4* out, size_t n4,
                                                             float w, StepParams p, int* __restrict__ flag) {
  constexpr bool kImage = FORM != kVtTune;
  const size_t tile = static_cast<size_t>(kBlock) * U;
  const size_t stride = static_cast<size_t>(gridDim.x) * tile;
  bool bad = false;
  size_t base = static_cast<size_t>(blockIdx.x) * tile;
  for (; base + tile <= n4; base += stride) {
    f32x4 vx[U], v0[U], vg[U], vs[U], vv[U], r[U], nv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (kImage) vx[u] = (NT & 4) ? __builtin_nontemporal_load(&x[i]) : x[i];
      vg[u] = __builtin_nontemporal_load(&g[i]);
      vs[u] = __builtin_nontemporal_load(&vsum[i]);
      vv[u] = v[i];
      if (FORM == kVtStep) v0[u] = __builtin_nontemporal_load(&x0[i]);
    }
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const f32x4 gh = vg[u] + vv[u];
      nv[u] = w * vs[u] - vg[u];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        r[u][k] = vt_image<FORM>(p, kImage ? vx[u][k] : 0.0f, gh[k], FORM == kVtStep ? v0[u][k] : 0.0f, bad);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (NT & 2) {
        __builtin_nontemporal_store(nv[u], &v[i]);
        __builtin_nontemporal_store(r[u], &out[i]);
      } else {
        v[i] = nv[u];
        out[i] = r[u];
      }
    }
  }
  if (base < n4) {                        // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < n4) {
        f32x4 vx, v0, r;
        if (kImage) vx = (NT & 4) ? __builtin_nontemporal_load(&x[i]) : x[i];
        const f32x4 vg = __builtin_nontemporal_load(&g[i]);
        const f32x4 vs = __builtin_nontemporal_load(&vsum[i]);
        const f32x4 vv = v[i];
        if (FORM == kVtStep) v0 = __builtin_nontemporal_load(&x0[i]);
        const f32x4 gh = vg + vv;
        const f32x4 nv = w * vs - vg;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          r[k] = vt_image<FORM>(p, kImage ? vx[k] : 0.0f, gh[k], FORM == kVtStep ? v0[k] : 0.0f, bad);
        if (NT & 2) {
          __builtin_nontemporal_store(nv, &v[i]);
          __builtin_nontemporal_store(r, &out[i]);
        } else {
          v[i] = nv;
          out[i] = r;
        }
      }
    }
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void vt_tune_scalar_kernel(const float* x, const float* g,
                                                                const float* __restrict__ vsum, float* v,
                                                                const float* __restrict__ x0, float* out, size_t n,
                                                                float w, StepParams p, int* __restrict__ flag) {
  constexpr bool kImage = FORM != kVtTune;
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float gi = g[i];
    const float gh = gi + v[i];
    v[i] = w * vsum[i] - gi;
    out[i] = vt_image<FORM>(p, kImage ? x[i] : 0.0f, gh, FORM == kVtStep ? x0[i] : 0.0f, bad);
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

inline bool vt_overlap(const void* a, size_t na, const void* b, size_t nb) {   // [a, a + na) meets [b, b + nb), bytes
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

template <int FORM>
static int launch_vt_tune(const float* x, const float* g, const float* vsum, float* v, const float* x0, float* out,
                          size_t n, float w, const StepParams& p, int* flag, vqa_stream_t stream) {
  constexpr bool kImage = FORM != kVtTune;
  if (!g || !vsum || !v || !out || (kImage && !x) || (FORM == kVtStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  if (n) {
    if (vt_overlap(g, nb, vsum, nb) || vt_overlap(g, nb, v, nb) || vt_overlap(vsum, nb, v, nb)) return VQA_ERR_SHAPE;
    if (vt_overlap(out, nb, vsum, nb) || vt_overlap(out, nb, v, nb)) return VQA_ERR_SHAPE;
    if (kImage ? vt_overlap(out, nb, g, nb) : (out != g && vt_overlap(out, nb, g, nb))) return VQA_ERR_SHAPE;
    if (FORM == kVtStep && vt_overlap(x0, nb, out, nb)) return VQA_ERR_SHAPE;
    if (FORM == kVtStep && vt_overlap(x0, nb, v, nb)) return VQA_ERR_SHAPE;
    if (kImage && x != out && vt_overlap(x, nb, out, nb)) return VQA_ERR_SHAPE;   // exactly in place, or apart
    if (kImage && vt_overlap(x, nb, v, nb)) return VQA_ERR_SHAPE;
  }
  if (!aligned4(g) || !aligned4(vsum) || !aligned4(v) || !aligned4(out) || (kImage && !aligned4(x)) ||
      (FORM == kVtStep && !aligned4(x0)))
    return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  const bool vec = (n % 4 == 0) && aligned16(g) && aligned16(vsum) && aligned16(v) && aligned16(out) &&
                   (!kImage || aligned16(x)) && (FORM != kVtStep || aligned16(x0));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!vec) {
    vt_tune_scalar_kernel<FORM><<<blocks_for(n, kBlock, cu_count() * 12), kBlock, 0, st>>>(x, g, vsum, v, x0, out, n, w,
                                                                                          p, flag);
    return launch_status();
  }
  constexpr int U = FORM == kVtTune ? 2 : 1;   // 3 read streams, or 4 / 5 with the image's: vt_unroll()
  const size_t n4 = n / 4;
  const int grid = blocks_for(n4, kBlock * U, cu_count() * 12);
  auto x4 = reinterpret_cast<const f32x4*>(x);
  auto g4 = reinterpret_cast<const f32x4*>(g);
  auto s4 = reinterpret_cast<const f32x4*>(vsum);
  auto v4 = reinterpret_cast<f32x4*>(v);
  auto z4 = reinterpret_cast<const f32x4*>(x0);
  auto o4 = reinterpret_cast<f32x4*>(out);
  int nt = kImage ? 4 : 0;
  if (nb > kVtNtStoreBytes) nt |= 2;
  if (x == out) nt &= ~4;
  // the tune form has no x stream: {0, 2}; the image forms {4, 6}, or {0, 2} in place
  if constexpr (kImage) {
    if ((nt & 6) == 4) {
      vt_tune_vec_kernel<FORM, U, 4><<<grid, kBlock, 0, st>>>(x4, g4, s4, v4, z4, o4, n4, w, p, flag);
      return launch_status();
    }
    if ((nt & 6) == 6) {
      vt_tune_vec_kernel<FORM, U, 6><<<grid, kBlock, 0, st>>>(x4, g4, s4, v4, z4, o4, n4, w, p, flag);
      return launch_status();
    }
  }
  if (nt & 2) vt_tune_vec_kernel<FORM, U, 2><<<grid, kBlock, 0, st>>>(x4, g4, s4, v4, z4, o4, n4, w, p, flag);
  else vt_tune_vec_kernel<FORM, U, 0><<<grid, kBlock, 0, st>>>(x4, g4, s4, v4, z4, o4, n4, w, p, flag);
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
  if (count < 1 || count > kVtMax || first < 0 || copy_stride < n) return VQA_ERR_SHAPE;
  const size_t span = (static_cast<size_t>(count - 1) * copy_stride + n) * sizeof(float);
  const size_t nb = n * sizeof(float);
  if (n && (vt_overlap(x, nb, out, span) || (m && vt_overlap(m, nb, out, span)) ||
            vt_overlap(key_dev, 3 * sizeof(unsigned), out, span)))
    return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || (m && !aligned4(m)) || !aligned4(key_dev)) return VQA_ERR_ALIGN;
  if (n == 0) return VQA_OK;
  const bool vec = (n % 4 == 0) && (copy_stride % 4 == 0) && aligned16(x) && aligned16(out) && (!m || aligned16(m));
  const bool nt_store = span > kVtNtStoreBytes;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t f = static_cast<uint32_t>(first);
  const uint64_t off = static_cast<uint64_t>(block_offset);
  if (m) launch_vt_neighbors<true>(count, vec, nt_store, st, x, m, out, n, copy_stride, f, off, bound, lookahead, key_dev);
  else launch_vt_neighbors<false>(count, vec, nt_store, st, x, nullptr, out, n, copy_stride, f, off, bound, lookahead, key_dev);
  return launch_status();
}

int vqa_vt_accumulate(const float* const* grads_host, int count, float* sum, size_t n, int init, vqa_stream_t stream) {
  clear_stale_error();
  if (!grads_host || !sum) return VQA_ERR_NULL;
  if (count < 1 || count > kVtMax) return VQA_ERR_SHAPE;
  for (int c = 0; c < count; ++c)
    if (!grads_host[c]) return VQA_ERR_NULL;
  const size_t nb = n * sizeof(float);
  for (int c = 0; c < count; ++c)
    if (n && vt_overlap(grads_host[c], nb, sum, nb)) return VQA_ERR_SHAPE;          // sum may alias no gradient
  if (!aligned4(sum)) return VQA_ERR_ALIGN;
  bool vec = (n % 4 == 0) && aligned16(sum);
  VtGrads a;
  for (int c = 0; c < kVtMax; ++c) {
    a.g[c] = c < count ? grads_host[c] : grads_host[0];
    if (!aligned4(a.g[c])) return VQA_ERR_ALIGN;
    vec = vec && aligned16(a.g[c]);
  }
  if (n == 0) return VQA_OK;
  const bool nt_store = nb > kVtNtStoreBytes;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (init) launch_vt_accumulate<true>(count, vec, nt_store, st, a, sum, n);
  else launch_vt_accumulate<false>(count, vec, nt_store, st, a, sum, n);
  return launch_status();
}

int vqa_vt_tune(const float* g, const float* vsum, float* v, float* ghat, size_t n, float w, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_vt_tune<kVtTune>(nullptr, g, vsum, v, nullptr, ghat, n, w, p, nullptr, stream);
}

int vqa_linf_vt_step(const float* x, const float* g, const float* vsum, float* v, const float* x0, float* out, size_t n,
                     float w, float eps_iter, float eps, float cmin, float cmax, unsigned mode, int* flag,
                     vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_vt_tune<kVtStep>(x, g, vsum, v, x0, out, n, w, p, flag, stream);
  return launch_vt_tune<kVtFgm>(x, g, vsum, v, nullptr, out, n, w, p, flag, stream);
}

}  // extern "C"
