// Translation-invariant (TI-FGSM, Dong et al., CVPR 2019) gradient smoothing, alone and fused with the L-infinity
// image update (gfx950 / MI355X).
//
// A separable K-tap stencil over every (H, W) plane of the gradient, zero padded (include/vqattack_hip.h has the
// contract: accumulators start at +0, taps in ascending order, one fp32 multiply and one fp32 add per term, rows first).
// One workgroup owns a 64 x TH output tile of one plane:
//   1. the tile and its r-wide halo of g go to LDS, out-of-plane positions as zeros (no address outside the plane is
//      formed), by dword loads, 8 in flight per lane;
//   2. the row pass writes a second LDS image (TH + K - 1 rows of 64): a lane makes 4 consecutive outputs from a sliding
//      register window, one new ds_read_b32 per tap.  The input image has an ODD row stride and a wave covers 8 groups
//      x 8 rows, so the 32 lanes the LDS serves together hit 32 different banks;
//   3. the column pass reads that image with one ds_read_b128 per tap and lane (4 consecutive outputs again) and feeds
//      the per-element body: a store (vqa_ti_smooth) or StepOp / FgmOp of common.hpp (vqa_linf_ti_step), whose x / x0
//      loads were issued before the pass.  The smoothed gradient of the fused form never reaches memory.
// K = 7 and K = 15 (the default) are compiled with the tap loops unrolled and the LDS images sized for them; every other
// K runs the same body with run-time loop bounds and images sized for K = 31.  -ffp-contract=off keeps the multiply and
// the add apart.
#include <limits.h>

#include "common.hpp"

namespace vqa {

constexpr int kTiMaxTaps = 31;
constexpr int kTiTileW = 64;                  // output tile width: 16 groups of 4
constexpr int kTiGroups = kTiTileW / 4;
constexpr int kTiLoads = 8;                   // dword loads of g in flight per lane while the tile is staged

// output tile height (VQA_KNOB: a compile-time constant in the shipped library): 32 or 64 rows.
// profiles/r20/README.md has the A/B.
VQA_KNOB g_opt_ti_tile_h = 32;

struct TiTaps {   // by value in the kernel arguments: no device allocation, no copy, capture-safe
  float w[kTiMaxTaps];
  int k;
};

enum { kTiSmooth = 0, kTiFgm = 1, kTiStep = 2 };

template <int TH, int KT>
struct TiTile {
  static constexpr int kMaxTaps = KT ? KT : kTiMaxTaps;
  static constexpr int kRows = TH + kMaxTaps - 1;                      // tile + halo rows
  static constexpr int kInStride = (kTiTileW + kMaxTaps - 1) | 1;      // odd: see the row pass
};

template <int TH, int KT, int FORM>
__global__ __launch_bounds__(kBlock) void ti_kernel(const float* __restrict__ g, const float* x,   // x may alias out
                                                    const float* __restrict__ x0, float* out, int height, int width,
                                                    int tiles_x, int tiles_y, TiTaps taps, StepParams p,
                                                    int* __restrict__ flag, int vec) {
  using T = TiTile<TH, KT>;
  __shared__ __attribute__((aligned(16))) float s_in[T::kRows * T::kInStride];
  __shared__ __attribute__((aligned(16))) float s_t[T::kRows * kTiTileW];
  const int K = KT ? KT : taps.k;
  const int r = K / 2;
  const int rows = TH + K - 1, cols = kTiTileW + K - 1;
  unsigned b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const size_t base = static_cast<size_t>(b / tiles_y) * height * width;      // this plane
  const int ox = tx * kTiTileW, oy = ty * TH;

  // 1. tile + halo -> LDS (the pad column of the odd stride included, as zero).  kTiLoads loads per lane are issued
  // back to back and WITHOUT a branch around them: behind a per-lane guard the compiler waits for every load before it
  // issues the next (one global latency per dword and lane, the whole kernel's time).  So a position outside the plane
  // loads the nearest element INSIDE it (the clamped coordinates: still no address outside the plane) and is then
  // replaced by zero; only the LDS stores of the last, partial round are guarded.
  const int total = rows * T::kInStride;
  for (int i0 = threadIdx.x; i0 < total; i0 += kBlock * kTiLoads) {
    float v[kTiLoads];
#pragma unroll
    for (int u = 0; u < kTiLoads; ++u) {
      const int i = i0 + u * kBlock;
      const int ly = i / T::kInStride, lx = i - ly * T::kInStride;
      const int gy = oy - r + ly, gx = ox - r + lx;
      const int cy = gy < 0 ? 0 : (gy < height ? gy : height - 1), cx = gx < 0 ? 0 : (gx < width ? gx : width - 1);
      const float t = g[base + static_cast<size_t>(cy) * width + cx];
      v[u] = (lx < cols && gy == cy && gx == cx) ? t : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kTiLoads; ++u) {
      const int i = i0 + u * kBlock;
      if (i < total) s_in[i] = v[u];
    }
  }
  __syncthreads();

  // 2. row pass: item -> (column half, row, group of the half); lanes 0..7 take 8 neighbouring groups of one row
  for (int it = threadIdx.x; it < rows * kTiGroups; it += kBlock) {
    const int q = it >> 3;
    const int half = q / rows, ry = q - half * rows;
    const int xg = (it & 7) + 8 * half;
    const float* src = s_in + ry * T::kInStride + xg * 4;
    float v0 = src[0], v1 = src[1], v2 = src[2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float v3 = src[j + 3];
      const float w = taps.w[j];
      a0 = a0 + w * v0;
      a1 = a1 + w * v1;
      a2 = a2 + w * v2;
      a3 = a3 + w * v3;
      v0 = v1, v1 = v2, v2 = v3;
    }
    *reinterpret_cast<f32x4*>(s_t + ry * kTiTileW + xg * 4) = f32x4{a0, a1, a2, a3};
  }
  __syncthreads();

  // 3. column pass + the per-element body
  bool bad = false;
  for (int it = threadIdx.x; it < TH * kTiGroups; it += kBlock) {
    const int ly = it / kTiGroups, xg = it % kTiGroups;
    const int gy = oy + ly, gx = ox + xg * 4;
    const bool live = gy < height && gx < width;
    const size_t off = base + static_cast<size_t>(gy) * width + gx;      // used only when live
    const int n = live ? (width - gx < 4 ? width - gx : 4) : 0;          // elements of this group inside the plane
    f32x4 xv = {0.0f, 0.0f, 0.0f, 0.0f}, x0v = xv;
    if (FORM != kTiSmooth && live) {
      if (vec) {               // every pointer 16-byte aligned and width % 4 == 0: the group is whole and aligned
        xv = *reinterpret_cast<const f32x4*>(x + off);
        if (FORM == kTiStep) x0v = *reinterpret_cast<const f32x4*>(x0 + off);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n) {
            xv[k] = x[off + k];
            if (FORM == kTiStep) x0v[k] = x0[off + k];
          }
        }
      }
    }
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* src = s_t + ly * kTiTileW + xg * 4;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const f32x4 tv = *reinterpret_cast<const f32x4*>(src + j * kTiTileW);
      const float w = taps.w[j];
      acc = acc + w * tv;
    }
    if (!live) continue;
    f32x4 res;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (FORM == kTiSmooth) res[k] = acc[k];
      else if (k >= n) res[k] = 0.0f;            // outside the plane: no body, so no range verdict on a value never loaded
      else if (FORM == kTiFgm) res[k] = FgmOp::apply(p, xv[k], acc[k], 0.0f, bad);
      else res[k] = StepOp::apply(p, xv[k], acc[k], x0v[k], bad);
    }
    if (vec) {
      *reinterpret_cast<f32x4*>(out + off) = res;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) out[off + k] = res[k];
    }
  }
  if (FORM != kTiSmooth && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, 1);
}

template <int TH, int FORM>
static void launch_ti_k(int grid, hipStream_t st, const float* g, const float* x, const float* x0, float* out, int height,
                        int width, int tiles_x, int tiles_y, const TiTaps& taps, const StepParams& p, int* flag, int vec) {
  if (taps.k == 15)
    ti_kernel<TH, 15, FORM><<<grid, kBlock, 0, st>>>(g, x, x0, out, height, width, tiles_x, tiles_y, taps, p, flag, vec);
  else if (taps.k == 7)
    ti_kernel<TH, 7, FORM><<<grid, kBlock, 0, st>>>(g, x, x0, out, height, width, tiles_x, tiles_y, taps, p, flag, vec);
  else
    ti_kernel<TH, 0, FORM><<<grid, kBlock, 0, st>>>(g, x, x0, out, height, width, tiles_x, tiles_y, taps, p, flag, vec);
}

// FORM kTiSmooth: x / x0 / flag unused.  Everything is validated before the first HIP call.
template <int FORM>
static int launch_ti(const float* g, const float* x, const float* x0, float* out, int planes, int height, int width,
                     const float* taps_host, int ktaps, const StepParams& p, int* flag, vqa_stream_t stream) {
  if (!g || !out || !taps_host || (FORM != kTiSmooth && !x)) return VQA_ERR_NULL;
  if (FORM != kTiSmooth && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (ktaps < 1 || ktaps > kTiMaxTaps || (ktaps & 1) == 0) return VQA_ERR_SHAPE;
  if (planes < 0 || height < 0 || width < 0) return VQA_ERR_SHAPE;
  if (g == out) return VQA_ERR_SHAPE;
  if (!aligned4(g) || !aligned4(out) || (x && !aligned4(x)) || (x0 && !aligned4(x0))) return VQA_ERR_ALIGN;
  if (planes == 0 || height == 0 || width == 0) return VQA_OK;
  const int th = g_opt_ti_tile_h;
  const unsigned long long tiles_x = (static_cast<unsigned long long>(width) + kTiTileW - 1) / kTiTileW;
  const unsigned long long tiles_y = (static_cast<unsigned long long>(height) + th - 1) / th;
  // one workgroup per tile in a one-dimensional grid: planes * tiles must fit its 31 bits (element offsets are size_t)
  if (tiles_x * tiles_y > static_cast<unsigned long long>(INT_MAX) / static_cast<unsigned long long>(planes))
    return VQA_ERR_SHAPE;
  const int grid = static_cast<int>(tiles_x * tiles_y * planes);
  TiTaps taps;
  for (int j = 0; j < kTiMaxTaps; ++j) taps.w[j] = j < ktaps ? taps_host[j] : 0.0f;
  taps.k = ktaps;
  const int vec = (width % 4 == 0) && aligned16(out) && (FORM == kTiSmooth || aligned16(x)) &&
                  (FORM != kTiStep || aligned16(x0));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tx = static_cast<int>(tiles_x), ty = static_cast<int>(tiles_y);
#ifdef VQA_TUNING
  if (th == 64) launch_ti_k<64, FORM>(grid, st, g, x, x0, out, height, width, tx, ty, taps, p, flag, vec);
  else
#endif
  launch_ti_k<32, FORM>(grid, st, g, x, x0, out, height, width, tx, ty, taps, p, flag, vec);
  return launch_status();
}

}  // namespace vqa

using namespace vqa;

extern "C" {

#ifdef VQA_TUNING
int vqa_ti_set_option(int value) {   // option 14 of vqa_set_option (linf.hip)
  if (value != 32 && value != 64) return VQA_ERR_SHAPE;
  g_opt_ti_tile_h = value;
  return VQA_OK;
}
#endif

int vqa_ti_smooth(const float* g, float* out, int planes, int height, int width, const float* taps_host, int ktaps,
                  vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_ti<kTiSmooth>(g, nullptr, nullptr, out, planes, height, width, taps_host, ktaps, p, nullptr, stream);
}

int vqa_linf_ti_step(const float* x, const float* g, const float* x0, float* out, int planes, int height, int width,
                     const float* taps_host, int ktaps, float eps_iter, float eps, float cmin, float cmax, unsigned mode,
                     int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_ti<kTiStep>(g, x, x0, out, planes, height, width, taps_host, ktaps, p, flag, stream);
  return launch_ti<kTiFgm>(g, x, nullptr, out, planes, height, width, taps_host, ktaps, p, flag, stream);
}

}  // extern "C"
