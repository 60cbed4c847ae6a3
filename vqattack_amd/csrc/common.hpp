// Shared device helpers for the gfx950 kernels of the VQAttack PGD path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vqattack_hip.h"

namespace vqa {

constexpr int kWave = 64;          // CDNA4 wavefront
constexpr int kBlock = 256;        // 4 waves per workgroup, one per SIMD
constexpr int kBlocksPerCu = 8;    // default grid cap of a grid-stride launch: 8 workgroups per compute unit (grid_cap())

// Launch-shape constants of the kernels.  The shipped library runs ONE variant, fixed at compile time (chosen from the
// sweeps recorded in DESIGN.md); a build with -DVQA_TUNING (tools/ only: `python -m vqattack_amd.build --tuning`) turns
// the constants into process-wide knobs behind vqa_set_option() and also compiles the alternatives the sweeps compare.
#ifdef VQA_TUNING
#define VQA_KNOB static int
#else
#define VQA_KNOB [[maybe_unused]] constexpr int
#endif

// torch.sign: (g > 0) - (g < 0); sign(+-0) = 0 and sign(NaN) = 0.
__device__ __forceinline__ float sign_torch(float g) {
  return (g > 0.0f ? 1.0f : 0.0f) - (g < 0.0f ? 1.0f : 0.0f);
}

// torch.clamp(v, lo, hi) = min(max(v, lo), hi) with NaN propagated (fminf/fmaxf drop NaN).
__device__ __forceinline__ float clamp_torch(float v, float lo, float hi) {
  float r = fminf(fmaxf(v, lo), hi);
  return (v != v) ? v : r;
}

__device__ __forceinline__ bool out_of_range(float v, float lo, float hi) {
  return !(v >= lo) || !(v <= hi);   // true for NaN, like torch.all(ge) / torch.all(le) failing
}

// The two L-infinity image updates that more than one file launches: linf.hip streams them over the gradient, the
// momentum step of lnorm.hip over the accumulated momentum -- one body, so the two cannot drift apart.
struct StepParams {
  float eps_iter, eps, cmin, cmax;
  unsigned mode;
};
struct FgmOp {   // out = clamp(x + eps_iter * sign(g))
  static constexpr int kIn = 2;
  __device__ static float apply(const StepParams& p, float x, float g, float, bool& bad) {
    if (p.mode & VQA_CHECK_RANGE) bad |= out_of_range(x, p.cmin, p.cmax);
    float v = x + p.eps_iter * sign_torch(g);
    return (p.mode & VQA_CLIP) ? clamp_torch(v, p.cmin, p.cmax) : v;
  }
};
struct StepOp {   // FGM update + projection on the eps-ball around x0
  static constexpr int kIn = 3;
  __device__ static float apply(const StepParams& p, float x, float g, float x0, bool& bad) {
    if (p.mode & VQA_CHECK_RANGE) bad |= out_of_range(x, p.cmin, p.cmax);
    float a = x + p.eps_iter * sign_torch(g);
    if (p.mode & VQA_CLIP) a = clamp_torch(a, p.cmin, p.cmax);
    float e = clamp_torch(a - x0, -p.eps, p.eps);
    float v = x0 + e;
    return (p.mode & VQA_CLIP) ? clamp_torch(v, p.cmin, p.cmax) : v;
  }
};

// The exact three-way bf16 split of an fp32 value (the bf16x6 products of gemm.hip and of the attention forward):
// a = a0 + a1 + a2 with a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1), both subtractions exact in fp32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// a -> (a0, a1, a2), exact for finite a whose bf16 rounding is finite.  Plain RNE casts (v_cvt_pk_bf16_f32).
// CHECKED: a0 = +-inf / NaN (a non-finite, or |a| at the top of the range rounding up) gets no correction terms, so
// that inf / NaN propagate through a product as in fp32 (the GEMMs).  Unchecked, such an element's a1 and a2 are NaN:
// for callers whose values are finite by construction or whose contract lets a non-finite input come out as NaN.
template <bool CHECKED = true>
__device__ __forceinline__ void split2(f32x2 a, bf16x2& h0, bf16x2& h1, bf16x2& h2) {
  h0 = __builtin_convertvector(a, bf16x2);
  f32x2 r = a - __builtin_convertvector(h0, f32x2);
  if (CHECKED) {
    r.x = __builtin_isfinite(r.x) ? r.x : 0.0f;
    r.y = __builtin_isfinite(r.y) ? r.y : 0.0f;
  }
  h1 = __builtin_convertvector(r, bf16x2);
  h2 = __builtin_convertvector(r - __builtin_convertvector(h1, f32x2), bf16x2);
}

template <bool CHECKED = true>
__device__ __forceinline__ void split8(const f32x4& lo, const f32x4& hi, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
  bf16x2 a[4], b[4], c[4];
  split2<CHECKED>(f32x2{lo.x, lo.y}, a[0], b[0], c[0]);
  split2<CHECKED>(f32x2{lo.z, lo.w}, a[1], b[1], c[1]);
  split2<CHECKED>(f32x2{hi.x, hi.y}, a[2], b[2], c[2]);
  split2<CHECKED>(f32x2{hi.z, hi.w}, a[3], b[3], c[3]);
  p0 = bf16x8{a[0].x, a[0].y, a[1].x, a[1].y, a[2].x, a[2].y, a[3].x, a[3].y};
  p1 = bf16x8{b[0].x, b[0].y, b[1].x, b[1].y, b[2].x, b[2].y, b[3].x, b[3].y};
  p2 = bf16x8{c[0].x, c[0].y, c[1].x, c[1].y, c[2].x, c[2].y, c[3].x, c[3].y};
}

// Cross-lane reductions on the DPP path (v_add_f32_dpp / v_max_f32_dpp: one VALU op per step, no LDS crossbar
// traffic and no lgkmcnt wait, unlike __shfl_xor which lowers to ds_bpermute_b32 on gfx9): two quad permutes, the
// two row mirrors, then row_bcast:15 / row_bcast:31 funnel the four 16-lane rows into lane 63, which is broadcast
// through an SGPR.  Every lane returns the same bits; the summation order is fixed, so results are reproducible.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                               CTRL, ROW_MASK, 0xF, false));
}
constexpr int kDppQuadSwap1 = 0xB1;     // quad_perm:[1,0,3,2]
constexpr int kDppQuadSwap2 = 0x4E;     // quad_perm:[2,3,0,1]
constexpr int kDppRowHalfMirror = 0x141;
constexpr int kDppRowMirror = 0x140;
constexpr int kDppRowBcast15 = 0x142;
constexpr int kDppRowBcast31 = 0x143;

__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_move<kDppQuadSwap1, 0xF>(0.0f, v);
  v += dpp_move<kDppQuadSwap2, 0xF>(0.0f, v);
  v += dpp_move<kDppRowHalfMirror, 0xF>(0.0f, v);
  v += dpp_move<kDppRowMirror, 0xF>(0.0f, v);
  v += dpp_move<kDppRowBcast15, 0xA>(0.0f, v);   // rows 1 and 3 += last lane of rows 0 and 2
  v += dpp_move<kDppRowBcast31, 0xC>(0.0f, v);   // rows 2 and 3 += lane 31
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_move<kDppQuadSwap1, 0xF>(v, v));
  v = fmaxf(v, dpp_move<kDppQuadSwap2, 0xF>(v, v));
  v = fmaxf(v, dpp_move<kDppRowHalfMirror, 0xF>(v, v));
  v = fmaxf(v, dpp_move<kDppRowMirror, 0xF>(v, v));
  v = fmaxf(v, dpp_move<kDppRowBcast15, 0xA>(v, v));   // rows outside the mask keep `old` = v: max(v, v)
  v = fmaxf(v, dpp_move<kDppRowBcast31, 0xC>(v, v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- "last workgroup folds" arrival detection ------------------------------------------------------------------
// Every workgroup publishes its result with an agent-scope (write-through) store, drains it, and then counts itself in
// with RELAXED atomics -- no release fence, which would write back the whole L2 per workgroup.  Arrivals are counted
// in two levels (kArriveGroups group counters 64 bytes apart, then one top counter) so that at most ~grid/32 + 32
// same-address atomics serialise instead of `grid`.  Exactly one workgroup per launch gets `true`; it must issue an
// agent-scope acquire before reading what the others published, and call arrive_reset() when done.
// The counter block (kArriveWords unsigned) must be zero when the launch starts.
constexpr int kArriveGroups = 32;
constexpr int kArriveStride = 16;                                   // words between counters (64 bytes)
constexpr int kArriveWords = (kArriveGroups + 1) * kArriveStride;

__device__ __forceinline__ bool arrive_is_last(unsigned* counters) {    // call from ONE thread per workgroup
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // the published stores have left this CU
  const unsigned grid = gridDim.x;
  const unsigned g = blockIdx.x % kArriveGroups;
  const unsigned members = grid / kArriveGroups + (g < grid % kArriveGroups ? 1u : 0u);
  const unsigned prev = __hip_atomic_fetch_add(counters + g * kArriveStride, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  if (prev + 1 != members) return false;
  const unsigned groups = grid < kArriveGroups ? grid : kArriveGroups;
  const unsigned top = __hip_atomic_fetch_add(counters + kArriveGroups * kArriveStride, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
  return top + 1 == groups;
}

__device__ __forceinline__ void arrive_reset(unsigned* counters) {      // by the folding workgroup, any of its threads
  for (int i = threadIdx.x; i <= kArriveGroups; i += blockDim.x)
    __hip_atomic_store(counters + i * kArriveStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// Compute units of the current device, queried once per device (MI355X: 256).
inline int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

inline int grid_cap() { return cu_count() * kBlocksPerCu; }

inline int blocks_for(size_t work_items, int per_block, int cap = 0) {      // cap <= 0: grid_cap()
  if (cap <= 0) cap = grid_cap();
  size_t b = (work_items + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > static_cast<size_t>(cap)) b = cap;
  return static_cast<int>(b);
}

// Workgroups of `kernel` that are resident at once on the whole device (occupancy x CUs): the grid of a persistent /
// grid-stride kernel, so that no workgroup waits for a slot and the last wave of workgroups is not part-empty.
template <class K>
inline int resident_blocks(K kernel, int block_threads, int fallback_per_cu) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, 0) != hipSuccess || per_cu <= 0)
    per_cu = fallback_per_cu;
  return per_cu * cu_count();
}

// hipGetLastError() is sticky across calls: an entry point first drops whatever an unrelated earlier HIP call left
// behind, so that launch_status() reports THIS launch only.
inline void clear_stale_error() { (void)hipGetLastError(); }

inline int launch_status() { return static_cast<int>(hipGetLastError()); }

}  // namespace vqa
