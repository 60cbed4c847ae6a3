// Per-sample norm reductions and the L2 / L1 image updates (gfx950 / MI355X).
//
// Reductions are two-stage and deterministic: stage 1 (grid = chunks x batch) reduces a contiguous chunk of one
// sample with 16-byte loads -> wave shuffle (DPP) reduction -> 4-wave LDS combine and writes ONE partial per
// workgroup; stage 2 (one workgroup per sample) folds the partials in index order.  No float atomics, so the
// norms -- and therefore the perturbations -- are bitwise reproducible from run to run.
// The update kernels re-read the gradient; at the path's sizes (<= 453 MB per tensor) that second read is mostly
// served by the 256 MiB Infinity Cache when the batch is small and by HBM otherwise (algorithmic bytes are
// counted as HBM bytes either way).
#include "stream.hpp"

namespace vqa {

constexpr int kRedU = 4;                 // 16-byte loads in flight per lane
constexpr int kMaxChunks = 512;          // partials per sample (stage 2 folds them with one workgroup)

static int chunks_for(int batch, size_t n_per) {
  size_t per_block = static_cast<size_t>(kBlock) * kRedU * 4;   // elements one workgroup covers per sweep
  size_t c = (n_per + per_block - 1) / per_block;
  size_t cap = static_cast<size_t>(grid_cap()) * 2 / (batch > 0 ? batch : 1);
  if (cap < 1) cap = 1;
  if (cap > kMaxChunks) cap = kMaxChunks;
  if (c > cap) c = cap;
  if (c < 1) c = 1;
  return static_cast<int>(c);
}

__device__ __forceinline__ float block_sum(float v, float* lds) {
  v = wave_sum(v);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) lds[w] = v;
  __syncthreads();
  float r = lds[0];
#pragma unroll
  for (int i = 1; i < kBlock / kWave; ++i) r += lds[i];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float block_max(float v, float* lds) {
  v = wave_max(v);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) lds[w] = v;
  __syncthreads();
  float r = lds[0];
#pragma unroll
  for (int i = 1; i < kBlock / kWave; ++i) r = fmaxf(r, lds[i]);
  __syncthreads();
  return r;
}

// A workgroup's share of one sample: elements [lo, hi) with lo a multiple of 4.
__device__ __forceinline__ void chunk_bounds(size_t n_per, int chunks, size_t& lo, size_t& hi) {
  size_t n4 = (n_per + 3) / 4;
  size_t per = (n4 + chunks - 1) / chunks;
  lo = static_cast<size_t>(blockIdx.x) * per * 4;
  hi = lo + per * 4;
  if (lo > n_per) lo = n_per;
  if (hi > n_per) hi = n_per;
}

// ---- stage 1: sum of squares of (t - sub) -------------------------------------------------------
template <bool VEC, bool SUB>
__global__ __launch_bounds__(kBlock) void sumsq_stage1(const float* __restrict__ t, const float* __restrict__ sub,
                                                       float* __restrict__ ws, size_t n_per, int chunks) {
  __shared__ float lds[kBlock / kWave];
  const size_t base = static_cast<size_t>(blockIdx.y) * n_per;
  size_t lo, hi;
  chunk_bounds(n_per, chunks, lo, hi);
  float acc = 0.0f;
  if (VEC) {
    const f32x4* t4 = reinterpret_cast<const f32x4*>(t + base);
    const f32x4* s4 = reinterpret_cast<const f32x4*>(sub + (SUB ? base : 0));
    const size_t lo4 = lo / 4, hi4 = hi / 4;   // VEC requires n_per % 4 == 0
    for (size_t i = lo4 + threadIdx.x; i < hi4; i += static_cast<size_t>(kBlock) * kRedU) {
      f32x4 v[kRedU], s[kRedU];
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t j = i + static_cast<size_t>(u) * kBlock;
        if (j < hi4) {
          v[u] = t4[j];
          if (SUB) s[u] = s4[j];
        }
      }
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t j = i + static_cast<size_t>(u) * kBlock;
        if (j < hi4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float d = SUB ? (v[u][k] - s[u][k]) : v[u][k];
            acc += d * d;
          }
        }
      }
    }
  } else {
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) {
      float d = SUB ? (t[base + i] - sub[base + i]) : t[base + i];
      acc += d * d;
    }
  }
  float r = block_sum(acc, lds);
  if (threadIdx.x == 0) ws[static_cast<size_t>(blockIdx.y) * chunks + blockIdx.x] = r;
}

__global__ __launch_bounds__(kBlock) void sum_stage2(const float* __restrict__ ws, float* __restrict__ out,
                                                     int chunks) {
  __shared__ float lds[kBlock / kWave];
  const float* p = ws + static_cast<size_t>(blockIdx.x) * chunks;
  float acc = 0.0f;
  for (int i = threadIdx.x; i < chunks; i += kBlock) acc += p[i];
  float r = block_sum(acc, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// ---- stage 1/2: max |g| and the number of elements attaining it ---------------------------------
// Stage 1 reads its chunk from HBM exactly once: the chunk is swept in register-resident tiles (kTieU 16-byte pieces per
// lane); per tile the workgroup reduces the maximum and counts the elements that attain it from the SAME registers,
// then merges (max, count) into the chunk's running pair -- no second sweep through L2.
constexpr int kTieU = 8;
template <bool VEC>
__global__ __launch_bounds__(kBlock) void absmax_stage1(const float* __restrict__ g, float* __restrict__ ws,
                                                        size_t n_per, int chunks, int batch) {
  __shared__ float lds[kBlock / kWave];
  const size_t base = static_cast<size_t>(blockIdx.y) * n_per;
  size_t lo, hi;
  chunk_bounds(n_per, chunks, lo, hi);
  // |g| >= 0.  fmaxf drops NaN; the reference's torch.max PROPAGATES it (the sample's maximum is NaN, nothing ties with
  // it, the result is 0 / 0 and the self-check assert of optimize_linear fires, utils.py:96-104): a NaN anywhere in the
  // chunk is tracked separately and makes the chunk's -- and so the sample's -- maximum NaN.
  float run_max = 0.0f, run_cnt = 0.0f, seen_nan = 0.0f;
  if (VEC) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + base);
    const size_t hi4 = hi / 4;
    for (size_t t0 = lo / 4; t0 < hi4; t0 += static_cast<size_t>(kBlock) * kTieU) {
      f32x4 v[kTieU];
      float m = 0.0f;
#pragma unroll
      for (int u = 0; u < kTieU; ++u) {
        const size_t j = t0 + static_cast<size_t>(u) * kBlock + threadIdx.x;
        v[u] = (j < hi4) ? g4[j] : f32x4{-1.0f, -1.0f, -1.0f, -1.0f};      // fabsf(-1) never ties with a tile max of 0
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j < hi4) {
            m = fmaxf(m, fabsf(v[u][k]));
            seen_nan = (v[u][k] != v[u][k]) ? 1.0f : seen_nan;
          }
      }
      const float tm = block_max(m, lds);
      float c = 0.0f;
#pragma unroll
      for (int u = 0; u < kTieU; ++u) {
        const size_t j = t0 + static_cast<size_t>(u) * kBlock + threadIdx.x;
        if (j < hi4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) c += (fabsf(v[u][k]) == tm) ? 1.0f : 0.0f;
        }
      }
      const float tc = block_sum(c, lds);
      if (tm > run_max) { run_max = tm; run_cnt = tc; }
      else if (tm == run_max) run_cnt += tc;
    }
  } else {
    float m = 0.0f;
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) {
      m = fmaxf(m, fabsf(g[base + i]));
      seen_nan = (g[base + i] != g[base + i]) ? 1.0f : seen_nan;
    }
    run_max = block_max(m, lds);
    float c = 0.0f;
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) c += (fabsf(g[base + i]) == run_max) ? 1.0f : 0.0f;
    run_cnt = block_sum(c, lds);
  }
  if (block_max(seen_nan, lds) > 0.0f) run_max = __builtin_nanf("");
  if (threadIdx.x == 0) {
    const size_t slot = static_cast<size_t>(blockIdx.y) * chunks + blockIdx.x;
    ws[slot] = run_max;
    ws[static_cast<size_t>(batch) * chunks + slot] = (lo < hi) ? run_cnt : 0.0f;
  }
}

__global__ __launch_bounds__(kBlock) void absmax_stage2(const float* __restrict__ ws, float* __restrict__ amax,
                                                        float* __restrict__ ties, int chunks, int batch) {
  __shared__ float lds[kBlock / kWave];
  const float* pm = ws + static_cast<size_t>(blockIdx.x) * chunks;
  const float* pc = ws + static_cast<size_t>(batch) * chunks + static_cast<size_t>(blockIdx.x) * chunks;
  float m = 0.0f, seen_nan = 0.0f;
  for (int i = threadIdx.x; i < chunks; i += kBlock) {
    m = fmaxf(m, pm[i]);
    seen_nan = (pm[i] != pm[i]) ? 1.0f : seen_nan;
  }
  float gm = block_max(m, lds);
  if (block_max(seen_nan, lds) > 0.0f) gm = __builtin_nanf("");       // torch.max propagates NaN
  float c = 0.0f;
  for (int i = threadIdx.x; i < chunks; i += kBlock) c += (pm[i] == gm) ? pc[i] : 0.0f;
  const float gc = block_sum(c, lds);
  if (threadIdx.x == 0) {
    amax[blockIdx.x] = gm;
    ties[blockIdx.x] = gc;
  }
}

// ---- per-sample elementwise updates -------------------------------------------------------------
struct NormParams {
  float eps, cmin, cmax;
  unsigned mode;
};

enum Kind { kL2Fgm, kL2Project, kL1Fgm, kClipEtaL2, kOptLinL2, kOptLinL1 };

// sqrt(max(1e-12, st)) and min(1, eps / length) as the reference forms them (A-ch/utils.py:33-37, :106-107): torch.max and
// torch.min PROPAGATE a NaN (a NaN sum of squares makes the whole sample NaN), fmaxf / fminf drop it.
__device__ __forceinline__ float l2_length(float st) { return sqrtf((st != st) ? st : fmaxf(1e-12f, st)); }
__device__ __forceinline__ float l2_factor(float eps, float st) {
  const float q = eps / l2_length(st);
  return (q != q) ? q : fminf(1.0f, q);
}

// s0/s1: the two element streams (x,g | adv,x0 | t,-); st/st2: per-sample statistics.
template <int KIND>
__device__ __forceinline__ float norm_apply(const NormParams& p, float a, float b, float st, float st2, bool& bad) {
  if (KIND == kL2Fgm) {
    if (p.mode & VQA_CHECK_RANGE) bad |= out_of_range(a, p.cmin, p.cmax);
    float v = a + p.eps * (b / l2_length(st));
    return (p.mode & VQA_CLIP) ? clamp_torch(v, p.cmin, p.cmax) : v;
  } else if (KIND == kL2Project) {
    float factor = l2_factor(p.eps, st);
    float v = b + (a - b) * factor;
    return (p.mode & VQA_CLIP) ? clamp_torch(v, p.cmin, p.cmax) : v;
  } else if (KIND == kL1Fgm) {
    if (p.mode & VQA_CHECK_RANGE) bad |= out_of_range(a, p.cmin, p.cmax);
    float hit = (fabsf(b) == st) ? 1.0f : 0.0f;
    float v = a + p.eps * (sign_torch(b) * hit / st2);
    return (p.mode & VQA_CLIP) ? clamp_torch(v, p.cmin, p.cmax) : v;
  } else if (KIND == kClipEtaL2) {
    return a * l2_factor(p.eps, st);
  } else if (KIND == kOptLinL2) {
    return p.eps * (a / l2_length(st));
  } else {
    float hit = (fabsf(a) == st) ? 1.0f : 0.0f;
    return p.eps * (sign_torch(a) * hit / st2);
  }
}

template <int KIND, bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void per_sample_kernel(const float* s0, const float* __restrict__ s1,
                                                            const float* __restrict__ stat,
                                                            const float* __restrict__ stat2, float* out,
                                                            size_t n_per, NormParams p, int* __restrict__ flag) {
  const size_t base = static_cast<size_t>(blockIdx.y) * n_per;
  const float st = stat[blockIdx.y];
  const float st2 = stat2 ? stat2[blockIdx.y] : 1.0f;
  bool bad = false;
  if (VEC) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(s0 + base);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(s1 + (TWO ? base : 0));
    f32x4* o4 = reinterpret_cast<f32x4*>(out + base);
    const size_t n4 = n_per / 4;
    const size_t tile = static_cast<size_t>(kBlock) * kRedU;
    for (size_t t0 = static_cast<size_t>(blockIdx.x) * tile; t0 < n4; t0 += static_cast<size_t>(gridDim.x) * tile) {
      f32x4 va[kRedU], vb[kRedU];
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t i = t0 + static_cast<size_t>(u) * kBlock + threadIdx.x;
        if (i < n4) {
          va[u] = a4[i];
          if (TWO) vb[u] = b4[i];
        }
      }
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t i = t0 + static_cast<size_t>(u) * kBlock + threadIdx.x;
        if (i < n4) {
          f32x4 r;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = norm_apply<KIND>(p, va[u][k], TWO ? vb[u][k] : 0.0f, st, st2, bad);
          o4[i] = r;
        }
      }
    }
  } else {
    for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_per;
         i += static_cast<size_t>(gridDim.x) * kBlock)
      out[base + i] = norm_apply<KIND>(p, s0[base + i], TWO ? s1[base + i] : 0.0f, st, st2, bad);
  }
  if ((p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
  // The reference's optimize_linear asserts that its result has unit norm (A-ch/utils.py:101-104 for L1, :110-116 for
  // L2) -- a host sync per call.  The assert can only fire when a sample's statistic is degenerate: L1: max|g| is 0 (all
  // entries tie with sign 0) or NaN; L2: the sum of squares is inf or NaN.  Reported as a flag bit instead.
  if (flag && blockIdx.x == 0 && threadIdx.x == 0) {
    bool degenerate = false;
    if (KIND == kL2Fgm || KIND == kOptLinL2) degenerate = !(st < INFINITY);
    if (KIND == kL1Fgm || KIND == kOptLinL1) degenerate = !(st > 0.0f) || !(st2 >= 1.0f);
    if (degenerate) atomicOr(flag, VQA_FLAG_DEGENERATE);
  }
}

template <int KIND, bool TWO>
static int launch_per_sample(const float* s0, const float* s1, const float* stat, const float* stat2, float* out,
                             int batch, size_t n_per, const NormParams& p, int* flag, vqa_stream_t stream) {
  if (!s0 || !out || !stat || (TWO && !s1)) return VQA_ERR_NULL;
  if ((KIND == kL1Fgm || KIND == kOptLinL1) && !stat2) return VQA_ERR_NULL;
  if ((p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535) return VQA_ERR_SHAPE;
  if (!aligned4(s0) || !aligned4(out) || (s1 && !aligned4(s1)) || !aligned4(stat) || (stat2 && !aligned4(stat2)) ||
      (flag && !aligned4(flag)))
    return VQA_ERR_ALIGN;
  if (batch == 0 || n_per == 0) return VQA_OK;
  const bool vec = (n_per % 4 == 0) && aligned16(s0) && aligned16(out) && (!TWO || aligned16(s1));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int gx = blocks_for(vec ? n_per / 4 : n_per, vec ? kBlock * kRedU : kBlock, grid_cap() / (batch < 8 ? batch : 8));
  dim3 grid(gx, batch);
  if (vec)
    per_sample_kernel<KIND, true, TWO><<<grid, kBlock, 0, st>>>(s0, s1, stat, stat2, out, n_per, p, flag);
  else
    per_sample_kernel<KIND, false, TWO><<<grid, kBlock, 0, st>>>(s0, s1, stat, stat2, out, n_per, p, flag);
  return launch_status();
}

// ---- momentum (MI-FGSM; cleverhans/tf2/attacks/momentum_iterative_method.py:88-95 of the reference tree) --------
// Per gradient evaluation and sample b:  den_b = max(1e-12, sum|g_b| / n);  m <- decay * m + g / den_b;  then the
// L-infinity update of linf.hip with m in place of g.  The sum is the two-stage scheme above with |.| for the square.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void sumabs_stage1(const float* __restrict__ g, float* __restrict__ ws,
                                                        size_t n_per, int chunks) {
  __shared__ float lds[kBlock / kWave];
  const size_t base = static_cast<size_t>(blockIdx.y) * n_per;
  size_t lo, hi;
  chunk_bounds(n_per, chunks, lo, hi);
  float acc = 0.0f;
  if (VEC) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + base);
    const size_t lo4 = lo / 4, hi4 = hi / 4;   // VEC requires n_per % 4 == 0
    for (size_t i = lo4 + threadIdx.x; i < hi4; i += static_cast<size_t>(kBlock) * kRedU) {
      f32x4 v[kRedU];
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t j = i + static_cast<size_t>(u) * kBlock;
        if (j < hi4) v[u] = g4[j];
      }
#pragma unroll
      for (int u = 0; u < kRedU; ++u) {
        const size_t j = i + static_cast<size_t>(u) * kBlock;
        if (j < hi4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc += fabsf(v[u][k]);
        }
      }
    }
  } else {
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += fabsf(g[base + i]);
  }
  float r = block_sum(acc, lds);
  if (threadIdx.x == 0) ws[static_cast<size_t>(blockIdx.y) * chunks + blockIdx.x] = r;
}

// 16-byte tiles in flight per lane and stream of the momentum kernels, chosen by register count (tools/isa_loop_mix.py
// --src lnorm.hip --waits).  The step form holds FOUR input streams: with 4 tiles it takes 120 registers (4 waves per
// SIMD; the form without x0 131: 3 waves) and the compiler starts storing before the last loads are back; with 2 tiles
// 63 / 43 registers, all 8 waves, every load of a tile issued before the first wait and the stores leaving together --
// and 8 waves x 8 loads keep the same 256 KB per CU in flight as 4 waves x 16.  A/B: profiles/r18/README.md.
VQA_KNOB g_opt_momentum_unroll = 2;
// The momentum is re-read by the next iteration, so it is loaded and stored plainly -- while it can stay in the 256 MB
// Infinity Cache.  1: a larger momentum (it cannot stay resident, and allocating its lines only costs bandwidth, as for
// `out`) is loaded and stored non-temporally; 0: always plain.  A/B: profiles/r18/README.md.
VQA_KNOB g_opt_momentum_nt_m = 1;

__device__ __forceinline__ float momentum_den(const float* __restrict__ sumabs, size_t n_per) {
  return fmaxf(1e-12f, sumabs[blockIdx.y] / static_cast<float>(n_per));    // workgroup-uniform: grid.y is the sample
}

// One element (or 16-byte piece): the momentum update (fp32 mul, IEEE div, add -- no contraction); the image update of
// stream.hpp follows on the new m.
template <class T>
__device__ __forceinline__ T momentum_update(float decay, float den, const T& m, const T& g) {
  return decay * m + g / den;
}

// grid = (tiles dealt round-robin, batch): den is uniform per workgroup and no 16-byte piece straddles two samples; the
// tile's pointers start at the sample.  FORM: kNoImage updates m only.
// g and x0 are read exactly once (non-temporal); NT bit1: non-temporal stores of `out`, NT bit2: non-temporal loads of
// x (never for an in-place update), NT bit3: non-temporal loads and stores of m (g_opt_momentum_nt_m, above).
template <int FORM, int NT>
struct MomentumTile {
  const f32x4* x;
  const f32x4* g;
  const f32x4* x0;
  f32x4* m;
  f32x4* out;
  size_t off;      // the sample's first piece
  float decay, den;
  StepParams p;
  struct Slot {
    f32x4 x = {}, g, x0 = {}, m;
  };
  __device__ __forceinline__ void load(Slot& s, size_t i) const {
    if (FORM != kNoImage) s.x = ld4<4, NT>(x + off + i);
    s.g = ld4_once(g + off + i);
    if (FORM == kStep) s.x0 = ld4_once(x0 + off + i);
    s.m = ld4<8, NT>(m + off + i);
  }
  __device__ __forceinline__ void compute(Slot& s, bool& bad) const {
    s.m = momentum_update(decay, den, s.m, s.g);
    if (FORM != kNoImage) s.x = image<FORM>(p, s.x, s.m, s.x0, bad);
  }
  static constexpr int kOutputs = FORM != kNoImage ? 2 : 1;
  __device__ __forceinline__ void store(const Slot& s, size_t i, int o) const {
    if (o == kOutputs - 1) st4<8, NT>(m + off + i, s.m);
    else st4<2, NT>(out + off + i, s.x);
  }
};

template <int FORM, int U, int NT>
__global__ __launch_bounds__(kBlock) void momentum_vec_kernel(const f32x4* x,   // may alias out
                                                              const f32x4* __restrict__ g,
                                                              const f32x4* __restrict__ x0, f32x4* m, f32x4* out,
                                                              const float* __restrict__ sumabs, size_t n_per,
                                                              float decay, StepParams p, int* __restrict__ flag) {
  const size_t n4 = n_per / 4;
  const MomentumTile<FORM, NT> t{x, g, x0, m, out, static_cast<size_t>(blockIdx.y) * n4, decay, momentum_den(sumabs, n_per), p};
  const bool bad = stream_tiles<U>(t, n4);
  if (FORM != kNoImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

// scalar path: n_per % 4 != 0 (sample boundaries fall inside 16-byte groups) or a pointer that is not 16-byte aligned
template <int FORM>
__global__ __launch_bounds__(kBlock) void momentum_scalar_kernel(const float* x, const float* __restrict__ g,
                                                                 const float* __restrict__ x0, float* m, float* out,
                                                                 const float* __restrict__ sumabs, size_t n_per,
                                                                 float decay, StepParams p, int* __restrict__ flag) {
  constexpr bool kImage = FORM != kNoImage;
  const size_t off = static_cast<size_t>(blockIdx.y) * n_per;
  const float den = momentum_den(sumabs, n_per);
  bool bad = false;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_per;
       i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float mi = momentum_update(decay, den, m[off + i], g[off + i]);
    if (kImage) out[off + i] = image<FORM>(p, x[off + i], mi, FORM == kStep ? x0[off + i] : 0.0f, bad);
    m[off + i] = mi;
  }
  if (kImage && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, VQA_FLAG_RANGE);
}

template <int FORM, int U>
static void launch_momentum_vec(int nt, dim3 grid, hipStream_t st, const float* x, const float* g, const float* x0,
                                float* m, float* out, const float* sumabs, size_t n_per, float decay,
                                const StepParams& p, int* flag) {
  auto x4 = reinterpret_cast<const f32x4*>(x);
  auto g4 = reinterpret_cast<const f32x4*>(g);
  auto z4 = reinterpret_cast<const f32x4*>(x0);
  auto m4 = reinterpret_cast<f32x4*>(m);
  auto o4 = reinterpret_cast<f32x4*>(out);
  // shipped hint sets: {0, 4} up to the Infinity Cache's size, {10, 14} above it (bit2 dropped for an in-place update);
  // the accumulate form has no image streams: {0, 8}
  switch (FORM == kNoImage ? (nt & 8) : (nt & 14)) {
#ifdef VQA_TUNING
    case 2: momentum_vec_kernel<FORM, U, 2><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
    case 6: momentum_vec_kernel<FORM, U, 6><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
#endif
    case 4: momentum_vec_kernel<FORM, U, 4><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
    case 8: momentum_vec_kernel<FORM, U, 8><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
    case 10: momentum_vec_kernel<FORM, U, 10><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
    case 14: momentum_vec_kernel<FORM, U, 14><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
    default: momentum_vec_kernel<FORM, U, 0><<<grid, kBlock, 0, st>>>(x4, g4, z4, m4, o4, sumabs, n_per, decay, p, flag); break;
  }
}

template <int FORM>
static int launch_momentum(const float* x, const float* g, const float* x0, float* m, float* out, const float* sumabs,
                           int batch, size_t n_per, float decay, const StepParams& p, int* flag, vqa_stream_t stream) {
  constexpr bool kImage = FORM != kNoImage;
  if (!g || !sumabs || !m || (kImage && (!x || !out)) || (FORM == kStep && !x0)) return VQA_ERR_NULL;
  if (kImage && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535) return VQA_ERR_SHAPE;
  if (!aligned4(g) || !aligned4(m) || !aligned4(sumabs) || (kImage && (!aligned4(x) || !aligned4(out))) ||
      (FORM == kStep && !aligned4(x0)))
    return VQA_ERR_ALIGN;
  if (batch == 0 || n_per == 0) return VQA_OK;
  const bool vec = (n_per % 4 == 0) && aligned16(g) && aligned16(m) && (!kImage || (aligned16(x) && aligned16(out))) &&
                   (FORM != kStep || aligned16(x0));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int unroll = g_opt_momentum_unroll;
  if (vec) {
    dim3 grid(stream_grid(n_per / 4, unroll, batch), batch);    // linf.hip's grid, dealt over the samples
    int nt = 4;                                                              // x is read once ...
    if (static_cast<size_t>(batch) * n_per * sizeof(float) > kInfinityCacheBytes)
      nt |= g_opt_momentum_nt_m ? 2 | 8 : 2;
    if (x == out) nt &= ~4;                                                  // ... unless it is about to be rewritten
#ifdef VQA_TUNING
    if (unroll == 4) launch_momentum_vec<FORM, 4>(nt, grid, st, x, g, x0, m, out, sumabs, n_per, decay, p, flag);
    else
#endif
    launch_momentum_vec<FORM, 2>(nt, grid, st, x, g, x0, m, out, sumabs, n_per, decay, p, flag);
  } else {
    dim3 grid(stream_grid(n_per, 1, batch), batch);
    momentum_scalar_kernel<FORM><<<grid, kBlock, 0, st>>>(x, g, x0, m, out, sumabs, n_per, decay, p, flag);
  }
  return launch_status();
}

}  // namespace vqa

using namespace vqa;

extern "C" {

#ifdef VQA_TUNING
int vqa_momentum_set_option(int value) {   // option 13 of vqa_set_option (linf.hip)
  if ((value & 7) != 2 && (value & 7) != 4) return VQA_ERR_SHAPE;   // tiles in flight | 8: non-temporal m above 256 MB
  g_opt_momentum_unroll = value & 7;
  g_opt_momentum_nt_m = (value & 8) ? 1 : 0;
  return VQA_OK;
}
#endif

int vqa_sumabs_per_sample(const float* g, float* out, int batch, size_t n_per_sample, float* ws, vqa_stream_t stream) {
  clear_stale_error();
  if (!g || !out || !ws) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535) return VQA_ERR_SHAPE;
  if (!aligned4(g) || !aligned4(out) || !aligned4(ws)) return VQA_ERR_ALIGN;
  if (batch == 0 || n_per_sample == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int chunks = chunks_for(batch, n_per_sample);
  dim3 grid(chunks, batch);
  if ((n_per_sample % 4 == 0) && aligned16(g))
    sumabs_stage1<true><<<grid, kBlock, 0, st>>>(g, ws, n_per_sample, chunks);
  else
    sumabs_stage1<false><<<grid, kBlock, 0, st>>>(g, ws, n_per_sample, chunks);
  sum_stage2<<<batch, kBlock, 0, st>>>(ws, out, chunks);
  return launch_status();
}

int vqa_momentum_accumulate(const float* g, const float* sumabs, float* m, int batch, size_t n_per_sample, float decay,
                            vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_momentum<kNoImage>(nullptr, g, nullptr, m, nullptr, sumabs, batch, n_per_sample, decay, p, nullptr,
                                         stream);
}

int vqa_linf_momentum_step(const float* x, const float* g, const float* sumabs, const float* x0, float* m, float* out,
                           int batch, size_t n_per_sample, float decay, float eps_iter, float eps, float cmin,
                           float cmax, unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_momentum<kStep>(x, g, x0, m, out, sumabs, batch, n_per_sample, decay, p, flag, stream);
  return launch_momentum<kFgm>(x, g, nullptr, m, out, sumabs, batch, n_per_sample, decay, p, flag, stream);
}

size_t vqa_reduce_ws_bytes(int batch, size_t n_per_sample) {
  if (batch <= 0) return 0;
  return static_cast<size_t>(batch) * chunks_for(batch, n_per_sample) * 2 * sizeof(float);
}

int vqa_sumsq_per_sample(const float* t, const float* sub, float* out, int batch, size_t n_per_sample, float* ws,
                         vqa_stream_t stream) {
  clear_stale_error();
  if (!t || !out || !ws) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535) return VQA_ERR_SHAPE;
  if (!aligned4(t) || (sub && !aligned4(sub)) || !aligned4(out) || !aligned4(ws)) return VQA_ERR_ALIGN;
  if (batch == 0 || n_per_sample == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int chunks = chunks_for(batch, n_per_sample);
  const bool vec = (n_per_sample % 4 == 0) && aligned16(t) && (!sub || aligned16(sub));
  dim3 grid(chunks, batch);
  if (vec && sub) sumsq_stage1<true, true><<<grid, kBlock, 0, st>>>(t, sub, ws, n_per_sample, chunks);
  else if (vec) sumsq_stage1<true, false><<<grid, kBlock, 0, st>>>(t, t, ws, n_per_sample, chunks);
  else if (sub) sumsq_stage1<false, true><<<grid, kBlock, 0, st>>>(t, sub, ws, n_per_sample, chunks);
  else sumsq_stage1<false, false><<<grid, kBlock, 0, st>>>(t, t, ws, n_per_sample, chunks);
  sum_stage2<<<batch, kBlock, 0, st>>>(ws, out, chunks);
  return launch_status();
}

int vqa_absmax_ties_per_sample(const float* g, float* amax, float* ties, int batch, size_t n_per_sample, float* ws,
                               vqa_stream_t stream) {
  clear_stale_error();
  if (!g || !amax || !ties || !ws) return VQA_ERR_NULL;
  if (batch < 0 || batch > 65535) return VQA_ERR_SHAPE;
  if (!aligned4(g) || !aligned4(amax) || !aligned4(ties) || !aligned4(ws)) return VQA_ERR_ALIGN;
  if (batch == 0 || n_per_sample == 0) return VQA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int chunks = chunks_for(batch, n_per_sample);
  dim3 grid(chunks, batch);
  if ((n_per_sample % 4 == 0) && aligned16(g))
    absmax_stage1<true><<<grid, kBlock, 0, st>>>(g, ws, n_per_sample, chunks, batch);
  else
    absmax_stage1<false><<<grid, kBlock, 0, st>>>(g, ws, n_per_sample, chunks, batch);
  absmax_stage2<<<batch, kBlock, 0, st>>>(ws, amax, ties, chunks, batch);
  return launch_status();
}

int vqa_l2_fgm(const float* x, const float* g, const float* sumsq_g, float* out, int batch, size_t n_per_sample,
               float eps_iter, float cmin, float cmax, unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  NormParams p{eps_iter, cmin, cmax, mode};
  return launch_per_sample<kL2Fgm, true>(x, g, sumsq_g, nullptr, out, batch, n_per_sample, p, flag, stream);
}

int vqa_l2_project(const float* adv, const float* x0, const float* sumsq_eta, float* out, int batch,
                   size_t n_per_sample, float eps, float cmin, float cmax, unsigned mode, vqa_stream_t stream) {
  clear_stale_error();
  NormParams p{eps, cmin, cmax, mode & ~VQA_CHECK_RANGE};
  return launch_per_sample<kL2Project, true>(adv, x0, sumsq_eta, nullptr, out, batch, n_per_sample, p, nullptr,
                                             stream);
}

int vqa_l1_fgm(const float* x, const float* g, const float* amax, const float* ties, float* out, int batch,
               size_t n_per_sample, float eps_iter, float cmin, float cmax, unsigned mode, int* flag,
               vqa_stream_t stream) {
  clear_stale_error();
  NormParams p{eps_iter, cmin, cmax, mode};
  return launch_per_sample<kL1Fgm, true>(x, g, amax, ties, out, batch, n_per_sample, p, flag, stream);
}

int vqa_scale_per_sample(const float* t, const float* stat, const float* stat2, float* out, int batch,
                         size_t n_per_sample, float eps, int kind, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  NormParams p{eps, 0.0f, 0.0f, 0u};
  switch (kind) {
    case 0: return launch_per_sample<kClipEtaL2, false>(t, nullptr, stat, nullptr, out, batch, n_per_sample, p, nullptr, stream);
    case 1: return launch_per_sample<kOptLinL2, false>(t, nullptr, stat, nullptr, out, batch, n_per_sample, p, flag, stream);
    case 2: return launch_per_sample<kOptLinL1, false>(t, nullptr, stat, stat2, out, batch, n_per_sample, p, flag, stream);
    default: return VQA_ERR_SHAPE;
  }
}

}  // extern "C"
