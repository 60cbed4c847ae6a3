// Input diversity (DI-FGSM, Xie et al., CVPR 2019): the per-sample bilinear shrink-and-pad transform, its adjoint, and
// the adjoint fused with the L-infinity image update (gfx950 / MI355X).
//
// One row [new_h, new_w, top, left] of a DEVICE int32 table describes a sample (include/vqattack_hip.h has the bit-level
// contract); a row outside its ranges is taken as the identity row [H, W, 0, 0].  Every kernel runs one 256-thread
// workgroup per 64 x 32 tile of one (H, W) plane; a lane owns groups of 4 consecutive pixels.
//   forward (di_forward_kernel): a destination pixel inside the window gathers its 2 x 2 source pixels with dword loads
//     (clamped into the plane, so no address outside it is formed) and blends them; +0 outside the window.
//   adjoint (di_adjoint_kernel), a gather without atomics.  For a tile of SOURCE pixels:
//     1. per axis, a table in LDS with two (destination index, weight) slots per source coordinate, filled by iterating
//        over the DESTINATION coordinates that can reach the tile with exactly the forward's arithmetic: destination d
//        puts (d, l0) into slot 1 of source i0 and (d, l1) into slot 0 of source i0 + 1.  i0 is strictly increasing in d,
//        so a slot is written at most once and slot 0's destination is the smaller one: ascending order for free;
//     2. the destination window rows / columns that those slots name (at most 65 + 2 columns and 33 + 2 rows: 65 / 33
//        values of i0 touch the tile, 2 for the rounding of the first candidate) go to LDS by dword loads, 5 in flight per
//        lane and no branch around them: a position outside the WINDOW loads the clamped, in-window address and becomes
//        zero, so nothing outside the window is ever read into the result;
//     3. the row pass t[dy, sx] goes into a second LDS image (a lane keeps one source column, its two slots in registers);
//     4. the column pass reads that image with one ds_read_b128 per slot and feeds the per-element body: a store
//        (vqa_di_adjoint) or StepOp / FgmOp of common.hpp (vqa_linf_di_step), whose x / x0 loads were issued before the
//        first barrier.  The image gradient of the fused form never reaches memory.
// An empty slot is skipped by a select, never multiplied by a zero weight.  -ffp-contract=off keeps multiply and add apart.
#include <limits.h>

#include "common.hpp"

namespace vqa {

constexpr int kDiTileW = 64;                    // tile width: 16 groups of 4
constexpr int kDiTileH = 32;
constexpr int kDiGroups = kDiTileW / 4;
constexpr int kDiItems = kDiTileH * kDiGroups / kBlock;      // groups of 4 per lane: 2
constexpr int kDiCols = kDiTileW + 4;           // staged destination columns: 65 contributors + 2 of slack, rounded up
constexpr int kDiRows = kDiTileH + 4;           // staged destination rows: 33 + 2, rounded up
constexpr int kDiStride = kDiCols | 1;          // odd row stride of the staged image
constexpr int kDiLoads = 5;                     // dword loads of gD in flight per lane: 2 rounds cover 36 x 69

enum { kDiAdjoint = 0, kDiFgm = 1, kDiStep = 2 };

struct DiGeom {
  int nh, nw, top, left;
};

// the sample's table row; anything outside the ranges is the identity row (the host wrappers refuse such tables)
__device__ __forceinline__ DiGeom di_geom(const int* __restrict__ geom, int sample, int height, int width) {
  DiGeom g{geom[4 * sample], geom[4 * sample + 1], geom[4 * sample + 2], geom[4 * sample + 3]};
  const bool ok = g.nh >= 1 && g.nh <= height && g.nw >= 1 && g.nw <= width && g.top >= 0 && g.top <= height - g.nh &&
                  g.left >= 0 && g.left <= width - g.nw;
  return ok ? g : DiGeom{height, width, 0, 0};
}

// one axis of the contract: destination d -> source i0, i0 + 1 with weights l0, l1
struct DiCoord {
  int i0;
  float l0, l1;
};
__device__ __forceinline__ DiCoord di_coord(float scale, int d) {
  const float src = scale * (static_cast<float>(d) + 0.5f) - 0.5f;
  const float f = floorf(src);
  DiCoord c;
  c.i0 = static_cast<int>(f);
  c.l1 = src - f;
  c.l0 = 1.0f - c.l1;
  return c;
}

// a destination coordinate at or below the first one whose i0 can be >= o - 1 (o: first source coordinate of the tile).
// The exact bound is (o - 0.5) / scale - 0.5; one is taken off for the fp32 rounding of this estimate.
__device__ __forceinline__ int di_first(float scale, int o) {
  const int q = static_cast<int>(floorf((static_cast<float>(o) - 0.5f) / scale - 0.5f)) - 1;
  return q < 0 ? 0 : q;
}

// Gather table of one axis for the source coordinates o .. o + len - 1: s_idx / s_w [2 * len], slot 0 then slot 1 per
// coordinate, index relative to d_lo (< span) or -1.  The caller has set every index to -1 and synchronised.
__device__ __forceinline__ void di_axis_table(int full, int nnew, int o, int len, int d_lo, int span, int* s_idx,
                                              float* s_w) {
  const float scale = static_cast<float>(full) / static_cast<float>(nnew);
  for (int j = threadIdx.x; j < span; j += kBlock) {
    const int d = d_lo + j;
    if (d >= nnew) continue;
    if (nnew == full) {                       // identity axis: one term, weight 1
      const int s = d - o;
      if (s >= 0 && s < len) {
        s_idx[2 * s + 1] = j;
        s_w[2 * s + 1] = 1.0f;
      }
      continue;
    }
    const DiCoord c = di_coord(scale, d);
    const int s0 = c.i0 - o, s1 = s0 + 1;
    if (s0 >= 0 && s0 < len && c.i0 < full) {
      s_idx[2 * s0 + 1] = j;
      s_w[2 * s0 + 1] = c.l0;
    }
    if (s1 >= 0 && s1 < len && c.i0 + 1 >= 0 && c.i0 + 1 < full) {
      s_idx[2 * s1] = j;
      s_w[2 * s1] = c.l1;
    }
  }
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void di_adjoint_kernel(const float* __restrict__ gd, const float* x,   // x may alias out
                                                            const float* __restrict__ x0, const int* __restrict__ geom,
                                                            float* out, int channels, int height, int width, int tiles_x,
                                                            int tiles_y, StepParams p, int* __restrict__ flag, int vec) {
  __shared__ __attribute__((aligned(16))) float s_t[kDiRows * kDiTileW];
  __shared__ float s_g[kDiRows * kDiStride];
  __shared__ int s_xi[2 * kDiTileW];
  __shared__ float s_xw[2 * kDiTileW];
  __shared__ int s_yi[2 * kDiTileH];
  __shared__ float s_yw[2 * kDiTileH];
  unsigned b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const int plane = b / tiles_y;
  const size_t base = static_cast<size_t>(plane) * height * width;
  const int ox = tx * kDiTileW, oy = ty * kDiTileH;
  const DiGeom gm = di_geom(geom, plane / channels, height, width);

  // x / x0 of this lane's groups: issued first, used last
  f32x4 xv[kDiItems], x0v[kDiItems];
  size_t off[kDiItems];
  int n[kDiItems];
#pragma unroll
  for (int u = 0; u < kDiItems; ++u) {
    const int it = threadIdx.x + u * kBlock;
    const int ly = it / kDiGroups, xg = it % kDiGroups;
    const int gy = oy + ly, gx = ox + xg * 4;
    const bool live = gy < height && gx < width;
    off[u] = base + static_cast<size_t>(gy) * width + gx;                 // used only when live
    n[u] = live ? (width - gx < 4 ? width - gx : 4) : 0;                  // elements of this group inside the plane
    xv[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    x0v[u] = xv[u];
    if (FORM != kDiAdjoint && live) {
      if (vec) {               // every pointer 16-byte aligned and width % 4 == 0: the group is whole and aligned
        xv[u] = *reinterpret_cast<const f32x4*>(x + off[u]);
        if (FORM == kDiStep) x0v[u] = *reinterpret_cast<const f32x4*>(x0 + off[u]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < n[u]) {
            xv[u][k] = x[off[u] + k];
            if (FORM == kDiStep) x0v[u][k] = x0[off[u] + k];
          }
        }
      }
    }
  }

  // 1. the gather tables
  if (threadIdx.x < 2 * kDiTileW) s_xi[threadIdx.x] = -1;
  if (threadIdx.x < 2 * kDiTileH) s_yi[threadIdx.x] = -1;
  const int dx0 = di_first(static_cast<float>(width) / static_cast<float>(gm.nw), ox);
  const int dy0 = di_first(static_cast<float>(height) / static_cast<float>(gm.nh), oy);
  __syncthreads();
  di_axis_table(width, gm.nw, ox, kDiTileW, dx0, kDiCols, s_xi, s_xw);
  di_axis_table(height, gm.nh, oy, kDiTileH, dy0, kDiRows, s_yi, s_yw);

  // 2. destination rows dy0.., columns dx0.. of the window -> LDS; outside the window: zero, from a clamped address
  const size_t wbase = base + static_cast<size_t>(gm.top) * width + gm.left;
  constexpr int total = kDiRows * kDiStride;
  for (int i0 = threadIdx.x; i0 < total; i0 += kBlock * kDiLoads) {
    float v[kDiLoads];
#pragma unroll
    for (int u = 0; u < kDiLoads; ++u) {
      const int i = i0 + u * kBlock;
      const int ly = i / kDiStride, lx = i - ly * kDiStride;
      const int dy = dy0 + ly, dx = dx0 + lx;
      const int cy = dy < gm.nh ? dy : gm.nh - 1, cx = dx < gm.nw ? dx : gm.nw - 1;
      const float t = gd[wbase + static_cast<size_t>(cy) * width + cx];
      v[u] = (lx < kDiCols && dy == cy && dx == cx) ? t : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kDiLoads; ++u) {
      const int i = i0 + u * kBlock;
      if (i < total) s_g[i] = v[u];
    }
  }
  __syncthreads();

  // 3. row pass: a lane keeps one source column
  {
    const int sx = threadIdx.x & (kDiTileW - 1);
    const int ia = s_xi[2 * sx], ib = s_xi[2 * sx + 1];
    const float wa = s_xw[2 * sx], wb = s_xw[2 * sx + 1];
    const int ca = ia < 0 ? 0 : ia, cb = ib < 0 ? 0 : ib;
    for (int ly = threadIdx.x / kDiTileW; ly < kDiRows; ly += kBlock / kDiTileW) {
      const float* row = s_g + ly * kDiStride;
      float acc = 0.0f;
      const float ta = wa * row[ca], tb = wb * row[cb];
      acc = ia < 0 ? acc : acc + ta;
      acc = ib < 0 ? acc : acc + tb;
      s_t[ly * kDiTileW + sx] = acc;
    }
  }
  __syncthreads();

  // 4. column pass + the per-element body
  bool bad = false;
#pragma unroll
  for (int u = 0; u < kDiItems; ++u) {
    const int it = threadIdx.x + u * kBlock;
    const int ly = it / kDiGroups, xg = it % kDiGroups;
    const int ia = s_yi[2 * ly], ib = s_yi[2 * ly + 1];
    const float wa = s_yw[2 * ly], wb = s_yw[2 * ly + 1];
    const f32x4 ta = *reinterpret_cast<const f32x4*>(s_t + (ia < 0 ? 0 : ia) * kDiTileW + xg * 4);
    const f32x4 tb = *reinterpret_cast<const f32x4*>(s_t + (ib < 0 ? 0 : ib) * kDiTileW + xg * 4);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ia >= 0) acc = acc + wa * ta;
    if (ib >= 0) acc = acc + wb * tb;
    if (n[u] == 0) continue;
    f32x4 res;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (FORM == kDiAdjoint) res[k] = acc[k];
      else if (k >= n[u]) res[k] = 0.0f;         // outside the plane: no body, so no range verdict on a value never loaded
      else if (FORM == kDiFgm) res[k] = FgmOp::apply(p, xv[u][k], acc[k], 0.0f, bad);
      else res[k] = StepOp::apply(p, xv[u][k], acc[k], x0v[u][k], bad);
    }
    if (vec) {
      *reinterpret_cast<f32x4*>(out + off[u]) = res;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n[u]) out[off[u] + k] = res[k];
    }
  }
  if (FORM != kDiAdjoint && (p.mode & VQA_CHECK_RANGE) && bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void di_forward_kernel(const float* __restrict__ x, const int* __restrict__ geom,
                                                            float* __restrict__ out, int channels, int height, int width,
                                                            int tiles_x, int tiles_y, int vec) {
  unsigned b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const int plane = b / tiles_y;
  const size_t base = static_cast<size_t>(plane) * height * width;
  const int ox = tx * kDiTileW, oy = ty * kDiTileH;
  const DiGeom gm = di_geom(geom, plane / channels, height, width);
  const float scale_x = static_cast<float>(width) / static_cast<float>(gm.nw);
  const float scale_y = static_cast<float>(height) / static_cast<float>(gm.nh);
  const bool ident_x = gm.nw == width, ident_y = gm.nh == height;
#pragma unroll
  for (int u = 0; u < kDiItems; ++u) {
    const int it = threadIdx.x + u * kBlock;
    const int ly = it / kDiGroups, xg = it % kDiGroups;
    const int gy = oy + ly, gx = ox + xg * 4;
    if (gy >= height || gx >= width) continue;
    const int n = width - gx < 4 ? width - gx : 4;
    const int dy = gy - gm.top;
    const bool in_y = dy >= 0 && dy < gm.nh;
    // source rows, clamped into the plane (the clamp is never taken for a valid row of the table)
    const DiCoord cy = di_coord(scale_y, in_y ? dy : 0);
    const int y0 = ident_y ? (in_y ? dy : 0) : (cy.i0 < 0 ? 0 : (cy.i0 < height ? cy.i0 : height - 1));
    const int y1 = y0 + 1 < height ? y0 + 1 : height - 1;
    const float* r0 = x + base + static_cast<size_t>(y0) * width;
    const float* r1 = x + base + static_cast<size_t>(y1) * width;
    f32x4 res;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int dx = gx + k - gm.left;
      const bool in = in_y && k < n && dx >= 0 && dx < gm.nw;
      const DiCoord cx = di_coord(scale_x, in ? dx : 0);
      const int x0i = ident_x ? (in ? dx : 0) : (cx.i0 < 0 ? 0 : (cx.i0 < width ? cx.i0 : width - 1));
      const int x1i = x0i + 1 < width ? x0i + 1 : width - 1;
      const float a = r0[x0i], bq = r0[x1i], c = r1[x0i], d = r1[x1i];
      const float top = ident_x ? a : cx.l0 * a + cx.l1 * bq;
      const float bot = ident_x ? c : cx.l0 * c + cx.l1 * d;
      const float v = ident_y ? top : cy.l0 * top + cy.l1 * bot;
      res[k] = in ? v : 0.0f;
    }
    const size_t off = base + static_cast<size_t>(gy) * width + gx;
    if (vec) {
      *reinterpret_cast<f32x4*>(out + off) = res;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) out[off + k] = res[k];
    }
  }
}

// grid of one workgroup per tile and plane; 0 when it does not fit the 31 bits of a one-dimensional grid
static int di_grid(int batch, int channels, int height, int width, int* tiles_x, int* tiles_y) {
  const unsigned long long tx = (static_cast<unsigned long long>(width) + kDiTileW - 1) / kDiTileW;
  const unsigned long long ty = (static_cast<unsigned long long>(height) + kDiTileH - 1) / kDiTileH;
  const unsigned long long planes = static_cast<unsigned long long>(batch) * static_cast<unsigned long long>(channels);
  if (planes > static_cast<unsigned long long>(INT_MAX) || tx * ty > static_cast<unsigned long long>(INT_MAX) / planes)
    return 0;
  *tiles_x = static_cast<int>(tx);
  *tiles_y = static_cast<int>(ty);
  return static_cast<int>(tx * ty * planes);
}

// FORM kDiAdjoint: x / x0 / flag unused.  Everything is validated before the first HIP call.
template <int FORM>
static int launch_di(const float* gd, const float* x, const float* x0, const int* geom, float* out, int batch,
                     int channels, int height, int width, const StepParams& p, int* flag, vqa_stream_t stream) {
  if (!gd || !out || !geom || (FORM != kDiAdjoint && !x)) return VQA_ERR_NULL;
  if (FORM != kDiAdjoint && (p.mode & VQA_CHECK_RANGE) && !flag) return VQA_ERR_NULL;
  if (batch < 0 || channels < 0 || height < 0 || width < 0) return VQA_ERR_SHAPE;
  if (gd == out) return VQA_ERR_SHAPE;
  if (!aligned4(gd) || !aligned4(out) || !aligned4(geom) || (x && !aligned4(x)) || (x0 && !aligned4(x0)))
    return VQA_ERR_ALIGN;
  if (batch == 0 || channels == 0 || height == 0 || width == 0) return VQA_OK;
  int tx = 0, ty = 0;
  const int grid = di_grid(batch, channels, height, width, &tx, &ty);
  if (grid == 0) return VQA_ERR_SHAPE;
  const int vec = (width % 4 == 0) && aligned16(out) && (FORM == kDiAdjoint || aligned16(x)) &&
                  (FORM != kDiStep || aligned16(x0));
  di_adjoint_kernel<FORM><<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(gd, x, x0, geom, out, channels, height,
                                                                                 width, tx, ty, p, flag, vec);
  return launch_status();
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_di_transform(const float* x, const int* geom, float* out, int batch, int channels, int height, int width,
                     vqa_stream_t stream) {
  clear_stale_error();
  if (!x || !out || !geom) return VQA_ERR_NULL;
  if (batch < 0 || channels < 0 || height < 0 || width < 0) return VQA_ERR_SHAPE;
  if (x == out) return VQA_ERR_SHAPE;
  if (!aligned4(x) || !aligned4(out) || !aligned4(geom)) return VQA_ERR_ALIGN;
  if (batch == 0 || channels == 0 || height == 0 || width == 0) return VQA_OK;
  int tx = 0, ty = 0;
  const int grid = di_grid(batch, channels, height, width, &tx, &ty);
  if (grid == 0) return VQA_ERR_SHAPE;
  const int vec = (width % 4 == 0) && aligned16(out);
  di_forward_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(x, geom, out, channels, height, width, tx, ty,
                                                                           vec);
  return launch_status();
}

int vqa_di_adjoint(const float* gd, const int* geom, float* out, int batch, int channels, int height, int width,
                   vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{0.0f, 0.0f, 0.0f, 0.0f, 0u};
  return launch_di<kDiAdjoint>(gd, nullptr, nullptr, geom, out, batch, channels, height, width, p, nullptr, stream);
}

int vqa_linf_di_step(const float* x, const float* gd, const float* x0, const int* geom, float* out, int batch,
                     int channels, int height, int width, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream) {
  clear_stale_error();
  StepParams p{eps_iter, eps, cmin, cmax, mode};
  if (x0) return launch_di<kDiStep>(gd, x, x0, geom, out, batch, channels, height, width, p, flag, stream);
  return launch_di<kDiFgm>(gd, x, nullptr, geom, out, batch, channels, height, width, p, flag, stream);
}

}  // extern "C"
