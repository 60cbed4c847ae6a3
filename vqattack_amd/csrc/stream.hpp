// The tile loop of the PGD path's HBM-bound stream kernels (linf.hip, lnorm.hip's momentum step, si.hip, admix.hip,
// vt.hip), written once, and the small launch rules and host-side checks those files share.  fold.hpp, on top of this
// header, holds the one kernel template that si.hip and admix.hip fold their gradient lists with.
//
// Such a kernel has arithmetic intensity < 0.5 flop/B: one 16-byte access per lane and stream, U slots of 256 pieces in
// flight per wave before the first use, 256-thread workgroups, a grid of 12 workgroups per CU that strides over
// block-contiguous tiles.  No LDS, no MFMA: there is no reuse to stage and no contraction.  A kernel supplies a Tile:
// a struct that holds the kernel's pointers and parameters, names the registers of one slot (`struct Slot`: a 16-byte
// piece of every stream) and has
//     void load(Slot& s, size_t i) const               read piece i of every input stream
//     void compute(Slot& s, bool& bad) const           the element chain, in registers; bad |= a failed range check
//     static constexpr int kOutputs                    output streams (or copies) per slot
//     void store(const Slot& s, size_t i, int o) const write piece i of output o
// The tile holds no registers of its own: a struct that mixed the kernel's arguments with slot arrays stays in memory
// until the slot loops are unrolled, and the code that comes out has other branches and waits (profiles/r26/README.md).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace vqa {

// ---- the loop -------------------------------------------------------------------------------------------------------
// Pieces [first, last) in tiles of U x 256, the tile starts `stride` apart (a multiple of the tile).
// Whole tiles first, in a loop of their own WITHOUT a branch around any load or store: the compiler counts a wave's
// outstanding loads and stores in one counter and, behind a per-lane `i < last` guard, no longer knows how many are
// younger than the one it needs -- the guarded form of this loop waited for the first of three loads before issuing the
// fourth, and for every store to be acknowledged before computing the next 16 bytes (tools/isa_loop_mix.py --src
// linf.hip --waits).  Here all of a tile's loads are issued back to back and consumed slot by slot, in order, with exact
// waits -- the scheduling barrier after each slot's arithmetic keeps the compiler from interleaving the slots, which
// costs registers and, where it starts with the last slot, waits for every load first -- and the tile's stores leave
// together, output stream by output stream.  Only the last tile of a range can be partial; it goes slot by slot: load,
// compute, store behind one guard.  Returns whether a range check failed.
template <int U, class Tile>
__device__ __forceinline__ bool stream_tiles(const Tile& t, size_t first, size_t last, size_t stride) {
  constexpr size_t tile = static_cast<size_t>(kBlock) * U;
  bool bad = false;
  size_t base = first;
  for (; base + tile <= last; base += stride) {
    typename Tile::Slot s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t.load(s[u], base + static_cast<size_t>(u) * kBlock + threadIdx.x);
    __builtin_amdgcn_sched_barrier(0);    // every load of the tile is in flight before the first one is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) {
      t.compute(s[u], bad);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int o = 0; o < Tile::kOutputs; ++o) {
#pragma unroll
      for (int u = 0; u < U; ++u) t.store(s[u], base + static_cast<size_t>(u) * kBlock + threadIdx.x, o);
    }
  }
  if (base < last) {                      // the partial tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kBlock + threadIdx.x;
      if (i < last) {
        typename Tile::Slot s;
        t.load(s, i);
        t.compute(s, bad);
#pragma unroll
        for (int o = 0; o < Tile::kOutputs; ++o) t.store(s, i, o);
      }
    }
  }
  return bad;
}

// The usual range: all n4 pieces, tiles dealt round-robin over grid.x.
template <int U, class Tile>
__device__ __forceinline__ bool stream_tiles(const Tile& t, size_t n4) {
  constexpr size_t tile = static_cast<size_t>(kBlock) * U;
  return stream_tiles<U>(t, static_cast<size_t>(blockIdx.x) * tile, n4, static_cast<size_t>(gridDim.x) * tile);
}

// ---- 16-byte accesses: non-temporal when bit BIT of the instance's NT mask is set -------------------------------------
template <int BIT, int NT>
__device__ __forceinline__ f32x4 ld4(const f32x4* p) {
  return (NT & BIT) ? __builtin_nontemporal_load(p) : *p;
}
template <int BIT, int NT>
__device__ __forceinline__ void st4(f32x4* p, const f32x4& v) {
  if (NT & BIT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}
__device__ __forceinline__ f32x4 ld4_once(const f32x4* p) { return ld4<1, 1>(p); }   // a stream that is read exactly once

// ---- element functions shared by the stages, on one float or on the four of a piece ----------------------------------
// What follows a stage's own arithmetic: nothing | FgmOp(x, g) | StepOp(x, g, x0).
enum ImageForm { kNoImage, kFgm, kStep };

template <int FORM>
__device__ __forceinline__ float image(const StepParams& p, float x, float g, float x0, bool& bad) {
  if (FORM == kStep) return StepOp::apply(p, x, g, x0, bad);
  if (FORM == kFgm) return FgmOp::apply(p, x, g, 0.0f, bad);
  return g;
}
template <int FORM>
__device__ __forceinline__ f32x4 image(const StepParams& p, const f32x4& x, const f32x4& g, const f32x4& x0, bool& bad) {
  if (FORM == kNoImage) return g;
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = image<FORM>(p, x[k], g[k], x0[k], bad);
  return r;
}

// The point the model is evaluated at: x, or the Nesterov look-ahead x + lookahead * m.
template <bool NI, class T>
__device__ __forceinline__ T lookahead_base(const T& x, const T& m, float lookahead) {
  return NI ? x + lookahead * m : x;
}

// ---- launch rules ---------------------------------------------------------------------------------------------------
// A result larger than the 256 MB Infinity Cache is stored non-temporally: a smaller one is re-read from the cache by the
// next kernel or the white box's next forward; a larger one cannot stay resident anyway and the plain-store allocation
// only costs bandwidth (tools/stream_probe, +10 % at 1.8 GB).
constexpr size_t kInfinityCacheBytes = 256ull << 20;

// 16-byte slots in flight per lane and stream, by register count (tools/isa_loop_mix.py --src si.hip): every read stream
// has an address of its own; two slots fit the 64 registers that keep 8 waves per SIMD up to 3 streams, one slot beyond
// -- which leaves the loads in flight per lane (slots x streams) about level over the stream counts.
constexpr int unroll_for(int streams) { return streams <= 3 ? 2 : 1; }

// Workgroups per CU in a stream kernel's grid.  Chosen when the L-infinity step kept 6 workgroups resident per CU (76
// registers): 12 = two whole rounds.  profiles/r06/step/step_ab.jsonl (tools/step_ab.py, alternating): batch 64 warm /
// after a cache flush 68.8 / 83.8 us at 12, 68.9 / 85.4 at 8 (previous build 69.6 / 87.0); batch 256 315.7 / 320.5 at
// 12, 318.4 / 321.7 at 8 (previous build 316.4 / 320.5) -- the memory system's ceiling either way.  With its slots
// consumed in order the step holds 64 registers and 8 workgroups per CU are resident (profiles/r26/README.md).
constexpr int kStreamBlocksPerCu = 12;

// grid.x for `items` pieces (or elements, U = 1: the scalar paths) in tiles of U x 256; `share`: the grid's y extent,
// over which the workgroups are dealt.
inline int stream_grid(size_t items, int U, int share = 1, int per_cu = kStreamBlocksPerCu) {
  int cap = cu_count() * per_cu / share;
  return blocks_for(items, kBlock * U, cap < 1 ? 1 : cap);
}

inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {   // [a, a + na) meets [b, b + nb)
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// `count` copies of n floats, copy_stride floats apart from `out` on, written in one launch from x, the optional m and the
// optional small device row `row` (row_bytes long).  VQA_ERR_SHAPE: copies that overlap each other or an input;
// VQA_ERR_ALIGN: a pointer that is not 4-byte aligned.  `bytes`: from the first copy's start to the last one's end;
// `vec`: whether the 16-byte kernel applies -- `unit`, the run of floats one workgroup row walks, is whole pieces too.
// The caller has checked its pointers for null and count >= 1.
struct CopiesSpan {
  size_t bytes = 0;
  bool vec = false;
};
inline int check_copies(CopiesSpan& s, const float* x, const float* m, const void* row, size_t row_bytes,
                        const float* out, size_t n, size_t unit, size_t copy_stride, int count) {
  if (copy_stride < n) return VQA_ERR_SHAPE;
  s.bytes = (static_cast<size_t>(count - 1) * copy_stride + n) * sizeof(float);
  const size_t nb = n * sizeof(float);
  if (n && (ranges_overlap(x, nb, out, s.bytes) || (m && ranges_overlap(m, nb, out, s.bytes)) ||
            (row && ranges_overlap(row, row_bytes, out, s.bytes))))
    return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || (m && !aligned4(m)) || !aligned4(row)) return VQA_ERR_ALIGN;
  s.vec = (unit % 4 == 0) && (copy_stride % 4 == 0) && aligned16(x) && aligned16(out) && (!m || aligned16(m));
  return VQA_OK;
}

// The host's list of `count` read streams of nb bytes as a by-value array of MAX: entries past count repeat the first
// (no instance reads them, and none is wild).  VQA_ERR_SHAPE: a count outside 1..MAX or a stream that meets `result`;
// VQA_ERR_NULL: a missing stream.  `low` collects the low address bits of the streams for the caller, which reports
// alignment behind overlap checks of its own: (low & 3) != 0 is VQA_ERR_ALIGN, (low & 15) != 0 the scalar path.
template <int MAX>
inline int pack_streams(const float* (&g)[MAX], uintptr_t& low, const float* const* host, int count, const void* result,
                        size_t nb) {
  if (count < 1 || count > MAX) return VQA_ERR_SHAPE;
  for (int c = 0; c < count; ++c)
    if (!host[c]) return VQA_ERR_NULL;
  for (int c = 0; c < count; ++c)
    if (nb && ranges_overlap(host[c], nb, result, nb)) return VQA_ERR_SHAPE;
  for (int c = 0; c < MAX; ++c) {
    g[c] = c < count ? host[c] : host[0];
    low |= reinterpret_cast<uintptr_t>(g[c]);
  }
  return VQA_OK;
}

// f(std::integral_constant<int, C>) with C = count clamped to 1..MAX: one kernel instance per count.
template <int MAX, class F>
inline void dispatch_count(int count, F&& f) {
  if constexpr (MAX > 1) {
    if (count < MAX) return dispatch_count<MAX - 1>(count, f);
  }
  f(std::integral_constant<int, MAX>{});
}

// f(std::integral_constant<int, NT>) with the NT mask of a kernel whose result takes `result_bytes`: bit1 = non-temporal
// stores (above), bit2 = non-temporal loads of the image x, which is read once -- unless the update is in place and x
// about to be rewritten.  A kernel without an image stream has the instances {0, 2}, one with {0, 2, 4, 6}.
template <bool IMAGE, class F>
inline void dispatch_nt(size_t result_bytes, bool in_place, F&& f) {
  const bool nt_store = result_bytes > kInfinityCacheBytes;
  if constexpr (IMAGE) {
    if (!in_place) {
      if (nt_store) f(std::integral_constant<int, 6>{});
      else f(std::integral_constant<int, 4>{});
      return;
    }
  }
  if (nt_store) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 0>{});
}

}  // namespace vqa
