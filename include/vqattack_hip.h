/*
 * vqattack_hip.h -- C ABI of the MI355X (gfx950) kernels behind VQAttack's PGD hot path.
 *
 * Boundary contract (last row): plain device pointers, element / row counts,
 * scalars and a hipStream_t; every entry point returns an int (0 = VQA_OK, otherwise a negative VQA_ERR_*
 * or a positive hipError_t), never allocates, never synchronises and never touches the host side of
 * its buffers, so a caller may capture any sequence of them into a hipGraph.  All tensors are fp32,
 * contiguous unless strides are passed explicitly.  "Reference" below is ericyinyzy/VQAttack; paths are
 * relative to its root, A-ch = ALBEF_VQAttack/cleverhans/cleverhans/torch, V-ch = the VLMO_VQAttack copy.
 *
 * The library is loaded by vqattack_amd/_hip.py (ctypes); INTEGRATION.md shows the stub a maintainer
 * of the reference would add to call it from the reference's own cleverhans modules.
 */
#ifndef VQATTACK_HIP_H
#define VQATTACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vqa_stream_t; /* a hipStream_t (NULL = the legacy default stream) */

#define VQA_OK 0
#define VQA_ERR_NULL (-1)     /* a required pointer is NULL */
#define VQA_ERR_SHAPE (-2)    /* a count/stride argument is out of the supported range */
#define VQA_ERR_ALIGN (-3)    /* a pointer that must be 4-byte aligned is not */

/* mode bits shared by the image-update entry points */
#define VQA_CLIP 1u           /* clamp the result to [cmin, cmax] (the reference's clip_min/clip_max not None) */
#define VQA_CHECK_RANGE 2u    /* atomically OR 1 into *flag when an INPUT x element is outside [cmin, cmax] or NaN
                                 (reference: torch.all(ge(x, clip_min)) / le(x, clip_max) sanity flags,
                                 A-ch/attacks/projected_gradient_descent.py:95-105) */
/* further bits the kernels may OR into a *flag word */
#define VQA_FLAG_RANGE 1      /* set by VQA_CHECK_RANGE */
#define VQA_FLAG_BAD_LABEL 2  /* vqa_ce_rows: a label is neither ignore_index nor in [0, V) (torch device-asserts) */
#define VQA_FLAG_DEGENERATE 4 /* optimize_linear self-check (A-ch/utils.py:101-104,110-116) would fail: norm=1 with a sample
                                 whose max |grad| is 0 or NaN, norm=2 with a non-finite sum of squares */

int vqa_abi_version(void);
const char* vqa_error_string(int code);

#ifdef VQA_TUNING
/* NOT part of the shipped library: libvqattack_hip.so runs one launch shape per kernel, fixed at compile time.  A build
 * with -DVQA_TUNING (`python -m vqattack_amd.build --tuning` -> lib/libvqattack_hip_tuning.so, used by tools/ only)
 * compiles the alternatives the sweeps of DESIGN.md compare and exposes them as process-wide knobs:
 *   option 0: resident workgroups per CU the grid is capped at (1..64, default 8)
 *   option 1: non-temporal hints, bit0 = gradient/second-stream loads, bit1 = result stores, bit2 = first/third-stream
 *             loads, bit3 = result stores only when the result exceeds the 256 MB Infinity Cache (default 1|4|8 = 13)
 *   option 2: 16-byte tiles in flight per lane and stream in vqa_linf_step (2, 4 or 8; default 4)
 *   option 3: tile-to-workgroup mapping, 0 = round-robin tiles (default), 1 = one contiguous chunk per workgroup
 *   option 4: workgroup size of the register-resident cross-entropy kernel (256, 512 or 1024; default 512)
 *   option 5: logits loads of the cross-entropy kernel, 2 = non-temporal only above 512 MB of logits (default),
 *             3 = always non-temporal (A/B measurements)
 *   option 6: grid of the cosine-loss kernel, 0 = exactly the resident workgroups (occupancy x CUs, default),
 *             n = 1..8 workgroups per CU
 *   option 7: rows in flight per wavefront in the cosine-loss kernel (1 or 2; default 2)
 *   option 8: non-temporal hints of the cosine-loss kernel, bit0 = loads of `a`, bit1 = gradient stores, bit2 = loads
 *             of the targets `b` (default 4)
 *   option 9: dQ-from-dS^T attention kernel, 1 = dS^T tile staged through LDS with 16-byte loads (default), 0 = direct
 *             dword loads into the MFMA operand (round 3's form)
 *   option 10: block-glue kernels, bit0 = non-temporal loads of the activation streams, bit1 = non-temporal stores of GELU
 *             results larger than the Infinity Cache (default 3)
 *   option 13: momentum kernels: 16-byte tiles in flight per lane and stream (2 or 4), + 8 = a momentum tensor larger
 *             than the Infinity Cache is loaded and stored non-temporally (default 2 + 8 = 10)
 *   option 14: output tile height of the TI smoothing kernels (32 or 64 rows of 64; default 32) */
int vqa_set_option(int option, int value);
#endif


/* ---------------------------------------------------------------- L-infinity image update (hot)
 * sign(g) follows torch.sign: sign(+-0) = 0, sign(NaN) = 0.  clamp propagates NaN like torch.clamp.
 * All four are pure elementwise streams; `out` may alias `x` (in-place) but no other aliasing.
 */

/* PGD start point: out = clamp(x + clamp(eta, -eps, eps), cmin, cmax); eta == NULL means eta = 0.
 * Replaces A-ch/attacks/projected_gradient_descent.py:110-120 (+ the range flags :95-105). 8-12 B/element. */
int vqa_linf_init(const float* x, const float* eta, float* out, size_t n, float eps, float cmin, float cmax,
                  unsigned mode, int* flag, vqa_stream_t stream);

/* FGM update only: out = clamp(x + eps_iter * sign(g), cmin, cmax).
 * Replaces A-ch/utils.py:86,127 + A-ch/attacks/fast_gradient_method.py:151-160. 12 B/element. */
int vqa_linf_fgm(const float* x, const float* g, float* out, size_t n, float eps_iter, float cmin, float cmax,
                 unsigned mode, int* flag, vqa_stream_t stream);

/* Fused PGD iteration tail (the north-star kernel): FGM update, then projection on the eps-ball around x0:
 *   a   = clamp(x + eps_iter * sign(g), cmin, cmax)
 *   e   = clamp(a - x0, -eps, eps)
 *   out = clamp(x0 + e, cmin, cmax)
 * Replaces rows 5-8 and 10-13 of SURVEY.md section 2.3 (A-ch/attacks/fast_gradient_method.py:151-160 +
 * A-ch/attacks/projected_gradient_descent.py:146-151). 16 B/element (reads x, g, x0; writes out). */
int vqa_linf_step(const float* x, const float* g, const float* x0, float* out, size_t n, float eps_iter,
                  float eps, float cmin, float cmax, unsigned mode, int* flag, vqa_stream_t stream);

/* Projection only: out = clamp(x0 + clamp(adv - x0, -eps, eps), cmin, cmax).
 * Replaces A-ch/attacks/projected_gradient_descent.py:146-151 on its own. 12 B/element. */
int vqa_linf_project(const float* adv, const float* x0, float* out, size_t n, float eps, float cmin,
                     float cmax, unsigned mode, vqa_stream_t stream);

/* clip_eta(norm=inf): out = clamp(eta, -eps, eps).  A-ch/utils.py:21. */
int vqa_clip_eta_linf(const float* eta, float* out, size_t n, float eps, vqa_stream_t stream);

/* optimize_linear(norm=inf): out = eps * sign(g).  A-ch/utils.py:86,127. */
int vqa_optimize_linear_linf(const float* g, float* out, size_t n, float eps, vqa_stream_t stream);

/* zero_out_clipped_grads: out = (x <= cmin && sign(grad) < 0) || (x >= cmax && sign(grad) > 0) ? 0 : grad.
 * A-ch/utils.py:131-149 (defined in the reference's utils, unused by its attack drivers). 12 B/element. */
int vqa_zero_out_clipped_grads(const float* grad, const float* x, float* out, size_t n, float cmin, float cmax,
                               vqa_stream_t stream);

/* ---------------------------------------------------------------- per-sample reductions (L2 / L1 norms)
 * Deterministic two-stage reductions: stage 1 writes per-block partials into `ws`, stage 2 combines them in a
 * fixed order, so results are bitwise reproducible run to run.  `ws` must hold vqa_reduce_ws_bytes() bytes.
 * Return codes of the reductions and of the L2 / L1 updates below, checked in this order: a required pointer NULL (`sub`,
 * `stat2` of kinds 0 / 1 and a `flag` without VQA_CHECK_RANGE are optional) VQA_ERR_NULL; batch outside 0..65535, or a
 * kind outside 0..2, VQA_ERR_SHAPE; any pointer -- statistics, workspace and flag included -- not 4-byte aligned
 * VQA_ERR_ALIGN; batch == 0 or n_per_sample == 0 VQA_OK, no launch.  A refused call writes nothing.  16-byte accesses
 * are used where n_per_sample % 4 == 0 and every element stream is 16-byte aligned, 4-byte accesses otherwise.
 * max(1e-12, s) and min(1, f) below are torch.max / torch.min: a NaN sum of squares stays NaN and makes its whole sample NaN.
 */
size_t vqa_reduce_ws_bytes(int batch, size_t n_per_sample);

/* out[b] = sum_i (t[b,i] - (sub ? sub[b,i] : 0))^2.   A-ch/utils.py:33-35 and :106. 4-8 B/element. */
int vqa_sumsq_per_sample(const float* t, const float* sub, float* out, int batch, size_t n_per_sample,
                         float* ws, vqa_stream_t stream);

/* amax[b] = max_i |g[b,i]|, ties[b] = #{i : |g[b,i]| == amax[b]}.  A-ch/utils.py:95-100.  */
int vqa_absmax_ties_per_sample(const float* g, float* amax, float* ties, int batch, size_t n_per_sample,
                               float* ws, vqa_stream_t stream);

/* FGM update, L2:  out = clamp(x + eps_iter * (g / sqrt(max(1e-12, sumsq_g[b]))), cmin, cmax).
 * A-ch/utils.py:106-107,127 + fast_gradient_method.py:152-160. */
int vqa_l2_fgm(const float* x, const float* g, const float* sumsq_g, float* out, int batch,
               size_t n_per_sample, float eps_iter, float cmin, float cmax, unsigned mode, int* flag,
               vqa_stream_t stream);

/* Projection, L2: eta = adv - x0; eta *= min(1, eps / sqrt(max(1e-12, sumsq_eta[b]))); out = clamp(x0 + eta).
 * A-ch/utils.py:31-39 + projected_gradient_descent.py:146-151. */
int vqa_l2_project(const float* adv, const float* x0, const float* sumsq_eta, float* out, int batch,
                   size_t n_per_sample, float eps, float cmin, float cmax, unsigned mode, vqa_stream_t stream);

/* FGM update, L1: out = clamp(x + eps_iter * sign(g) * [|g| == amax[b]] / ties[b], cmin, cmax).
 * A-ch/utils.py:88-101,127. */
int vqa_l1_fgm(const float* x, const float* g, const float* amax, const float* ties, float* out, int batch,
               size_t n_per_sample, float eps_iter, float cmin, float cmax, unsigned mode, int* flag,
               vqa_stream_t stream);

/* Per-sample scaling used by the stand-alone utils:
 *   kind 0 (clip_eta, norm=2):        out = t * min(1, eps / sqrt(max(1e-12, stat[b])))           A-ch/utils.py:31-39
 *   kind 1 (optimize_linear, norm=2): out = eps * (t / sqrt(max(1e-12, stat[b])))                 A-ch/utils.py:106-107,127
 *   kind 2 (optimize_linear, norm=1): out = eps * (sign(t) * [|t| == stat[b]] / stat2[b])         A-ch/utils.py:88-101,127
 * flag (nullable): kinds 1 and 2 OR VQA_FLAG_DEGENERATE into it when the reference's self-check assert of
 * optimize_linear (A-ch/utils.py:101-104, :110-116: the result must have unit norm) would fire for a sample; the same bit
 * is set by vqa_l2_fgm / vqa_l1_fgm when their flag pointer is given.  No host sync: the caller reads the word once.
 */
int vqa_scale_per_sample(const float* t, const float* stat, const float* stat2, float* out, int batch,
                         size_t n_per_sample, float eps, int kind, int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- momentum (MI-FGSM, Dong et al. 2017)
 * The reference tree ships the method for TensorFlow only (cleverhans/tf2/attacks/momentum_iterative_method.py); these
 * entry points give it to the torch operators.  Per gradient evaluation and sample b of n elements (:88-95 there):
 *   den_b = max(1e-12, sumabs[b] / (float)n)        grad / max(1e-12, reduce_mean(|grad|))     :91-94
 *   m    <- decay * m + g / den_b                   momentum = decay_factor * momentum + grad  :95
 * in fp32 with one rounding per operation (multiply, IEEE divide, add; no contraction).  The image update that follows
 * (:97-103) is this library's own chain with m in place of g.
 */

/* out[b] = sum_i |g[b,i]|: the two-stage reduction of vqa_sumsq_per_sample (same chunks, same workspace size), no
 * atomics, bitwise reproducible.  4 B/element. */
int vqa_sumabs_per_sample(const float* g, float* out, int batch, size_t n_per_sample, float* ws, vqa_stream_t stream);

/* m <- decay * m + g / den_b, in place.  The L2 loop runs it in front of vqa_l2_fgm(x, m, ...).  12 B/element. */
int vqa_momentum_accumulate(const float* g, const float* sumabs, float* m, int batch, size_t n_per_sample, float decay,
                            vqa_stream_t stream);

/* The accumulate above and the L-infinity update in ONE pass: m is updated in place, then out = vqa_linf_step(x, m, x0)
 * -- or, for x0 == NULL, out = vqa_linf_fgm(x, m) (no projection: the first sub-step of the dual-loss loop) -- bit for
 * bit what the two launches give.  24 B/element (reads x, g, x0, m; writes out, m), 20 without x0.  `out` may alias `x`;
 * mode / flag as in vqa_linf_step. */
int vqa_linf_momentum_step(const float* x, const float* g, const float* sumabs, const float* x0, float* m, float* out,
                           int batch, size_t n_per_sample, float decay, float eps_iter, float eps, float cmin,
                           float cmax, unsigned mode, int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- translation-invariant smoothing (TI-FGSM, Dong et al. 2019)
 * The reference tree has no TI in any framework; this definition is the contract.  For a gradient g of `planes` row-major
 * (height, width) planes and K = ktaps taps w[0..K-1] (K odd, 1 <= K <= 31, r = K / 2), per plane:
 *   t[y, x]    = sum_{j=0..K-1} w[j] * g[y, x + j - r]       (row pass)
 *   ghat[y, x] = sum_{j=0..K-1} w[j] * t[y + j - r, x]       (column pass)
 * Each accumulator starts at +0.0f, terms are taken in ascending j, each term is one fp32 multiply followed by one fp32
 * add (no contraction), planes are zero padded (a term whose source lies outside the plane adds w * 0) and never see
 * their neighbour planes.  K = 1, w = {1} gives g back with -0 as +0.  The paper's 2-D Gaussian kernel is the outer
 * product of its normalised 1-D taps, so the separable form is the same operator.
 * taps_host is a HOST pointer to K floats; they travel by value in the kernel arguments (no device allocation, no copy,
 * no sync: capture-safe like every other entry point).  One workgroup per 64 x 32 tile stages the tile and its halo in
 * LDS and runs both passes there.
 * Return codes, all before the first HIP call: a NULL g / out / x / taps_host, or VQA_CHECK_RANGE without flag,
 * VQA_ERR_NULL; ktaps even or outside 1..31, a negative extent, planes * tiles beyond the 2^31 - 1 workgroups of one
 * launch, or g == out, VQA_ERR_SHAPE; a pointer not 4-byte aligned VQA_ERR_ALIGN; any zero extent VQA_OK, no launch.
 * Pointers need 4-byte alignment only and width need not be a multiple of 4 (16-byte accesses are used where both allow).
 */

/* out = ghat.  8 B/element plus the halo re-reads of g (1.75 x at K = 15, mostly from L2).  g must not alias out. */
int vqa_ti_smooth(const float* g, float* out, int planes, int height, int width, const float* taps_host, int ktaps,
                  vqa_stream_t stream);

/* The smoothing above and the L-infinity update in ONE pass: out = vqa_linf_step(x, ghat, x0), or, for x0 == NULL,
 * out = vqa_linf_fgm(x, ghat) -- bit for bit what vqa_ti_smooth followed by that launch gives; ghat never goes to memory.
 * 16 B/element (12 without x0) plus the halo re-reads, against 24 for the two launches.  `out` may alias `x` (each
 * element of x is read only by the thread that writes it); g must not alias out.  mode / flag as in vqa_linf_step. */
int vqa_linf_ti_step(const float* x, const float* g, const float* x0, float* out, int planes, int height, int width,
                     const float* taps_host, int ktaps, float eps_iter, float eps, float cmin, float cmax, unsigned mode,
                     int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- input diversity (DI-FGSM, Xie et al. 2019)
 * The reference defines the transform for torch (cleverhans/fgsm_copy.py:9-31, `input_diversity`: a bilinear shrink to
 * (new_h, new_w) and zero padding back to (H, W) at a random offset) and never calls it.  Here it acts per sample on
 * every row-major (height, width) plane of a contiguous (batch, channels, height, width) tensor.  geom is a DEVICE
 * table of int32 rows [new_h, new_w, top, left], one per sample, with 1 <= new_h <= height, 1 <= new_w <= width,
 * 0 <= top <= height - new_h, 0 <= left <= width - new_w (a downscale only); it is read by the kernel, so a captured
 * launch sees whatever the table holds at replay.  A row outside these ranges is taken as the identity row
 * [height, width, 0, 0]; no flag is raised for it and no address outside the plane is formed, whatever the table holds.
 *
 * Per axis (full -> new), all in fp32, for destination coordinate d in 0 .. new - 1:
 *   scale = (float)full / (float)new;   src = scale * ((float)d + 0.5f) - 0.5f;
 *   i0 = floor(src);  i1 = i0 + 1;  l1 = src - (float)i0;  l0 = 1.0f - l1
 * (each operation rounded once, no contraction).  For new < full no clamp is needed: src >= 0, i1 <= full - 1 and i0 is
 * strictly increasing in d.  An axis with new == full is the identity on that axis: the single term i0 = d with weight
 * 1, and no term with a zero weight (so nothing at d + 1 is read).
 *
 * Forward, D = T(x): inside the new_h x new_w window at (top, left),
 *   D[top + dy, left + dx] = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d),
 *   a = x[y0, x0], b = x[y0, x1], c = x[y1, x0], d = x[y1, x1],
 * one fp32 multiply per product and one fp32 add per sum; on an identity axis the blend of that axis is its first
 * operand itself (x identity: a and c in place of the inner sums; y identity: the upper inner sum).  +0.0f outside the
 * window.  A source pixel that no destination references is not read into the result.
 *
 * Adjoint, g = T^T(gD), as a gather (deterministic, no atomics):
 *   t[dy, sx] = sum over the dx with i0(dx) == sx or i1(dx) == sx, in ascending dx, of wx * gD[top + dy, left + dx]
 *   g[sy, sx] = sum over the dy with i0(dy) == sy or i1(dy) == sy, in ascending dy, of wy * t[dy, sx]
 * where wx / wy is the l0 or l1 that the forward gives that pair (1 on an identity axis); each sum starts at +0.0f and
 * takes one fp32 multiply and one fp32 add per term.  A source coordinate has at most two contributors per axis (i0 is
 * strictly increasing); one with none gets +0.0f.  gD outside the window is never read into the result.  With the
 * identity row the adjoint returns gD with -0 as +0, the forward returns x bit for bit.
 *
 * One workgroup per 64 x 32 tile of one plane; the adjoint builds the per-axis (destination, weight) tables of its tile
 * in LDS from the forward's own arithmetic, stages the window rows it needs there and runs both passes on chip.
 * Return codes, all before the first HIP call: a NULL x / gD / geom / out, or VQA_CHECK_RANGE without flag,
 * VQA_ERR_NULL; a negative extent, batch * channels * tiles beyond the 2^31 - 1 workgroups of one launch, or the input
 * of the transform or of the adjoint being `out`, VQA_ERR_SHAPE; a pointer (geom included) not 4-byte aligned
 * VQA_ERR_ALIGN; any zero extent VQA_OK, no launch.  16-byte accesses are used where width % 4 == 0 and the pointers
 * allow.  No allocation, no copy, no sync: capture-safe.
 */

/* out = T(x).  8 B/element (the 2 x 2 gathers of x hit L1 / L2).  x must not alias out. */
int vqa_di_transform(const float* x, const int* geom, float* out, int batch, int channels, int height, int width,
                     vqa_stream_t stream);

/* out = T^T(gD): in front of vqa_ti_smooth, the momentum kernels and the L2 / L1 updates.  gD must not alias out. */
int vqa_di_adjoint(const float* gD, const int* geom, float* out, int batch, int channels, int height, int width,
                   vqa_stream_t stream);

/* The adjoint above and the L-infinity update in ONE pass: out = vqa_linf_step(x, T^T(gD), x0), or, for x0 == NULL,
 * out = vqa_linf_fgm(x, T^T(gD)) -- bit for bit what vqa_di_adjoint followed by that launch gives; the image gradient
 * never goes to memory.  At most 16 B/element (12 without x0; gD is read inside the window only), against 24 for the
 * two launches.  `out` may alias `x` (each element of x is read only by the thread that writes it); gD must not alias
 * out.  mode / flag as in vqa_linf_step. */
int vqa_linf_di_step(const float* x, const float* gD, const float* x0, const int* geom, float* out, int batch,
                     int channels, int height, int width, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- scale copies and Nesterov look-ahead (SI-NI-FGSM, Lin et al. 2020)
 * The reference tree has neither in any framework; this definition is the contract.  Per gradient evaluation the model
 * sees `copies` scaled images s_i * (x [+ lookahead * m]) (the paper: s_i = 2^-i, lookahead = eps_iter * decay, m the
 * momentum; no clamp and no projection, the authors' code looks ahead unclipped) and the image gradient is
 *   ghat = sum_i w_i * g_i,   w_i = s_i / copies  (the paper's average and the chain rule through the scaling),
 * all in fp32 with one rounding per operation (no contraction).  At most VQA_SI_MAX_COPIES copies.  Scales, weights
 * and the list of gradient pointers are HOST arrays that travel by value in the kernel arguments (no device allocation,
 * no copy, no sync: capture-safe; the gradient addresses are then fixed in a captured launch).  16-byte accesses are
 * used when n % 4 == 0 (and copy_stride % 4 == 0) and every pointer, each gradient included, is 16-byte aligned.
 * Return codes, all before the first HIP call: a NULL required pointer, a NULL entry of grads_host, or VQA_CHECK_RANGE
 * without flag, VQA_ERR_NULL; copies outside 1..VQA_SI_MAX_COPIES, copy_stride < n, or a forbidden overlap or alias,
 * VQA_ERR_SHAPE; a pointer not 4-byte aligned VQA_ERR_ALIGN; n == 0 VQA_OK, no launch.
 */
#define VQA_SI_MAX_COPIES 8
int vqa_si_max_copies(void);

/* out[i * copy_stride + e] = s_i * x[e] for m == NULL, else s_i * (x[e] + lookahead * m[e]) (multiply, add, multiply),
 * i < copies, e < n.  s = 1 with m == NULL is a bit copy of x.  One launch reads x (and m) once and writes every copy:
 * 4 (+ 4) + 4 * copies B/element.  copy_stride >= n; out must not overlap x or m. */
int vqa_si_copies(const float* x, const float* m, float* out, size_t n, size_t copy_stride, const float* scales_host,
                  int copies, float lookahead, vqa_stream_t stream);

/* out[e] = acc, acc = w_0 * g_0[e], then acc = acc + w_i * g_i[e] for i = 1 .. copies - 1 ascending.  The accumulator
 * starts from the first product, not from +0: copies = 1, w = {1} is the exact identity, signed zeros included.
 * grads_host is a HOST array of `copies` DEVICE pointers.  4 * copies + 4 B/element.  out may alias no gradient. */
int vqa_si_combine(const float* const* grads_host, const float* weights_host, int copies, float* out, size_t n,
                   vqa_stream_t stream);

/* The combination above and the L-infinity update in ONE pass: out = vqa_linf_step(x, ghat, x0), or, for x0 == NULL,
 * out = vqa_linf_fgm(x, ghat) -- bit for bit what vqa_si_combine followed by that launch gives; ghat never goes to
 * memory.  4 * copies + 12 B/element (8 without x0) against (4 * copies + 4) + 16 for the two launches.  `out` may be
 * exactly `x` (in place) and must not otherwise overlap x, x0 or a gradient.  mode / flag as in vqa_linf_step. */
int vqa_linf_si_step(const float* x, const float* const* grads_host, const float* weights_host, int copies,
                     const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin, float cmax,
                     unsigned mode, int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- mixed-image copies (Admix, Wang et al. 2021)
 * The reference tree has it in no framework; this definition is the contract.  Per gradient evaluation the model sees
 * m2 GROUPS of `copies` scaled images; group j mixes every sample b with another sample partner_j[b] of the batch:
 *   v = (x[b] [+ lookahead * m[b]]) + eta * x[partner_j[b]],   leaf_{j,i}[b] = s_i * v
 * (the paper: eta = 0.2, s_i = 2^-i, 5 copies, 3 groups; the partner is read from x itself, without the look-ahead; no
 * clamp and no projection), and the image gradient is the running sum over the groups in ascending j, copies ascending,
 *   gsum = sum_j sum_i w_i * g_{j,i},   w_i = s_i / (copies * m2),
 * group 0 through vqa_si_combine (the sum starts from its first product, not from +0), every later group continuing it
 * through the entry points below -- all in fp32 with one rounding per operation (no contraction).  At most
 * VQA_SI_MAX_COPIES copies per group and launch.  Scales, weights and the list of gradient pointers are HOST arrays that
 * travel by value in the kernel arguments, as for SI (capture-safe: no allocation, no copy, no sync); the partner row is
 * read from DEVICE memory, so that a captured launch sees whatever the row holds at each replay.  16-byte accesses are
 * used when per % 4 == 0 and copy_stride % 4 == 0 (the copies), n % 4 == 0 (the sums), and every pointer, each gradient
 * included, is 16-byte aligned.  Return codes, all before the first HIP call: a NULL required pointer, a NULL entry of
 * grads_host, or VQA_CHECK_RANGE without flag, VQA_ERR_NULL; copies outside 1..VQA_SI_MAX_COPIES, batch outside
 * 0..65535, copy_stride < batch * per, or a forbidden overlap or alias, VQA_ERR_SHAPE; a pointer not 4-byte aligned
 * VQA_ERR_ALIGN; no element VQA_OK, no launch.
 */

/* The `copies` scaled copies of ONE group: out[i * copy_stride + b * per + e] = s_i * v with v as above (multiply, add
 * for the look-ahead; multiply for eta * partner; add; multiply), i < copies, b < batch, e < per.  partner: a DEVICE row
 * of `batch` int32; an entry outside [0, batch) never addresses memory, it stands for b itself.  One launch reads x
 * twice (as itself and as a partner; the second read comes from the Infinity Cache) and m once and writes every copy:
 * 4 (+ 4) + 4 + 4 * copies B/element.  copy_stride >= batch * per; out must not overlap x, m or the partner row. */
int vqa_admix_copies(const float* x, const float* m, const int* partner, float* out, int batch, size_t per,
                     size_t copy_stride, const float* scales_host, int copies, float eta, float lookahead,
                     vqa_stream_t stream);

/* acc[e] = a, a = acc[e], then a = a + w_i * g_i[e] for i = 0 .. copies - 1 ascending, exactly in place: vqa_si_combine
 * on group 0 followed by this on the groups 1 .. m2 - 1 is the sum above.  grads_host is a HOST array of `copies` DEVICE
 * pointers.  4 * copies + 8 B/element.  acc may alias no gradient. */
int vqa_admix_accumulate(float* acc, const float* const* grads_host, const float* weights_host, int copies, size_t n,
                         vqa_stream_t stream);

/* The same sum and the L-infinity update in ONE pass: out = vqa_linf_step(x, a, x0), or, for x0 == NULL,
 * out = vqa_linf_fgm(x, a) -- bit for bit what vqa_admix_accumulate followed by that launch gives; neither the sum nor
 * acc is written.  4 * copies + 16 B/element (12 without x0) against (4 * copies + 8) + 16 for the two launches.  `out`
 * may be exactly `x` (in place) and must not otherwise overlap x, x0, acc or a gradient.  mode / flag as in
 * vqa_linf_step. */
int vqa_linf_admix_step(const float* x, const float* acc, const float* const* grads_host, const float* weights_host,
                        int copies, const float* x0, float* out, size_t n, float eps_iter, float eps, float cmin,
                        float cmax, unsigned mode, int* flag, vqa_stream_t stream);

/* ---------------------------------------------------------------- variance tuning (VMI / VNI-FGSM, Wang & He 2021)
 * The reference tree has it in no framework; this definition is the contract.  Let G(p) be the image gradient of one
 * evaluation at p (after the SI combination and the DI adjoint, before TI smoothing).  Evaluation t at point p steps
 * along  ghat = G(p) + v  and then sets  v <- w * (G(p + r_0) + G(p + r_1) + ... + G(p + r_{N-1})) - G(p),
 * w = fp32(1) / fp32(N), the sum in ascending i starting from G(p + r_0) (not from +0), v = 0 before the first
 * evaluation; r_i ~ U[-bound, bound) per element, bound = fp32(beta * eps), neighbours unclipped as in the authors'
 * code.  All in fp32 with one rounding per operation (no contraction).
 *
 * The random numbers are Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85):
 *   key     = (seed & 0xffffffff, seed >> 32)                of a 64-bit seed,
 *   counter = (j & 0xffffffff, j >> 32, i, t),               j = block_offset + e / 4 for flat element index e,
 *                                                            i the neighbour index, t the evaluation index,
 * and output word e % 4 belongs to element e:
 *   u = float(word >> 8) * 2^-24;  r = (u * 2 - 1) * bound  (only the last product rounds);  out = base + r.
 * An element's value depends on (seed, t, i, e, block_offset) alone -- not on the vector or scalar path, the grid,
 * the unroll or how the neighbours are grouped into launches.  Known answers (counter | key | output):
 *   0 0 0 0 | 0 0 | 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ffffffff x 4 | ffffffff x 2 | 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   243f6a88 85a308d3 13198a2e 03707344 | a4093822 299f31d0 | d16cfe09 94fdcceb 5001e420 24126ea1
 *
 * Capture-safe like the rest: no allocation, no copy, no sync; gradient pointer lists are HOST arrays that travel by
 * value in the kernel arguments (as for SI); seed and t are read from DEVICE memory, so that a captured launch sees
 * whatever the row holds at each replay.  16-byte accesses when n % 4 == 0 (and copy_stride % 4 == 0) and every pointer
 * is 16-byte aligned.  Return codes, all before the first HIP call: a NULL required pointer, a NULL entry of
 * grads_host, or VQA_CHECK_RANGE without flag, VQA_ERR_NULL; a count outside 1..VQA_VT_MAX_CHUNK, first < 0,
 * copy_stride < n, or a forbidden overlap or alias, VQA_ERR_SHAPE; a pointer not 4-byte aligned VQA_ERR_ALIGN; n == 0
 * VQA_OK, no launch.
 */
#define VQA_VT_MAX_CHUNK 8
int vqa_vt_max_chunk(void);

/* Neighbours first .. first + count - 1 of one evaluation: out[c * copy_stride + e] = base[e] + r_{first + c}[e], with
 * base = x for m == NULL, else x + lookahead * m (multiply, add: the Nesterov point), and r as above.  key_dev: a DEVICE
 * row of three uint32 (seed_lo, seed_hi, t).  One launch reads x (and m) once: 4 (+ 4) + 4 * count B/element.
 * copy_stride >= n; out must not overlap x, m or the key row. */
int vqa_vt_neighbors(const float* x, const float* m, float* out, size_t n, size_t copy_stride, int count, int first,
                     unsigned long long block_offset, float bound, float lookahead, const unsigned* key_dev,
                     vqa_stream_t stream);

/* sum[e] = acc, acc = init ? g_0[e] : sum[e] + g_0[e], then acc = acc + g_i[e] for i = 1 .. count - 1 ascending:
 * calling it with 8 pointers once or with 1 pointer eight times gives the same bits.  grads_host is a HOST array of
 * `count` DEVICE pointers.  4 * count + 4 (+ 4) B/element.  sum may alias no gradient. */
int vqa_vt_accumulate(const float* const* grads_host, int count, float* sum, size_t n, int init, vqa_stream_t stream);

/* ghat[e] = g[e] + v[e];  v[e] = w * vsum[e] - g[e]  (multiply, subtract), the old v in the first, 20 B/element.
 * ghat may be exactly g; v is updated in place; no other overlap among g, vsum, v, ghat. */
int vqa_vt_tune(const float* g, const float* vsum, float* v, float* ghat, size_t n, float w, vqa_stream_t stream);

/* The tune step above and the L-infinity update in ONE pass: out = vqa_linf_step(x, ghat, x0), or, for x0 == NULL,
 * out = vqa_linf_fgm(x, ghat) -- bit for bit what vqa_vt_tune followed by that launch gives; ghat never goes to memory.
 * 28 B/element (24 without x0) against 20 + 16 for the two launches.  `out` may be exactly `x` (in place) and must not
 * otherwise overlap x, x0, g, vsum or v.  mode / flag as in vqa_linf_step. */
int vqa_linf_vt_step(const float* x, const float* g, const float* vsum, float* v, const float* x0, float* out, size_t n,
                     float w, float eps_iter, float eps, float cmin, float cmax, unsigned mode, int* flag,
                     vqa_stream_t stream);

/* ---------------------------------------------------------------- cross-modal loss reduction
 * Rows of D contiguous floats, addressed as row(o, i) = base + o*stride0 + i*stride1 (strides in ELEMENTS) for
 * o < rows0, i < rows1 -- this is how the reference's `out[k][:, :feat_len, :]` truncation views are consumed
 * without a copy.  For every row pair:  c = sum_d (a_d / max(|a|, cos_eps)) * (b_d / max(|b|, cos_eps))
 * (torch.nn.CosineSimilarity semantics of torch 2.x).  The kernel accumulates  -c  per block into
 * partial[] and, when ga != NULL, writes d(gscale * sum(-c)) / d a  into ga (same addressing as a, with its own
 * strides) -- loss value and the gradient w.r.t. the model output in ONE pass over a and b.
 * row_mask (nullable, uint8 row WEIGHTS): row (o, i) is weighted by w = row_mask[(o % mask_period) * rows1 + i];
 * w == 0 rows contribute nothing and get a zero gradient whatever they hold, NaN included (padded text tokens of a
 * batched adapter; they must be readable: the kernel for rows of 256, 512, ... floats reads them), w == 2 counts a
 * row twice (the VLMO loss takes the [CLS] row both on its own and as a token, V-ch/attacks/fast_gradient_method.py:111).
 * Replaces nn.CosineSimilarity + negate + two torch.sum calls and their autograd backward:
 * A-ch/attacks/fast_gradient_method.py:98,120-127; V-ch/attacks/fast_gradient_method.py:102-114.
 * D must be a multiple of 4 and <= 2048; a, b, ga 16-byte aligned with strides multiples of 4.
 * Algorithmic bytes: 8*D per row (loss only) or 12*D per row (loss + gradient).
 * `partial` must hold vqa_neg_cos_partials() floats: one slot per workgroup plus the arrival counter of the in-kernel
 * fold, which must be ZERO before the first launch that uses the buffer (the folding workgroup resets it; launches that
 * share a buffer must be ordered on one stream).
 * loss_out (nullable): the workgroup that arrives last folds the partials in index order and writes
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + gscale * sum(partial)      -- bitwise reproducible, no second launch.
 * loss_out == NULL: partials only; fold them with vqa_sum_partials(partial, vqa_neg_cos_partials(), ...).
 * The grid is the number of workgroups resident at once (occupancy x compute units, queried from the device).
 */
int vqa_neg_cos_partials(void);
int vqa_neg_cos_rows(const float* a, const float* b, float* ga, float* partial, const uint8_t* row_mask,
                     long mask_period, long rows0, long rows1, int D, long a_stride0, long a_stride1,
                     long b_stride0, long b_stride1, long g_stride0, long g_stride1, float gscale,
                     float cos_eps, float* loss_out, int accumulate, vqa_stream_t stream);

/* The same pass over n_layers <= vqa_neg_cos_max_layers() feature maps of identical shape and strides in ONE launch
 * (the 13 / 25 per-layer maps of an encoder, never packed into one tensor): a, b, ga are HOST arrays of n_layers device
 * base pointers, copied into the kernel arguments (capture-safe); ga == NULL -> loss only.  Replaces the reference's
 * torch.cat / torch.stack feature packing (ALBEF_attack/adv_attack.py:124-125, vlmo_module.py:1435-1444) together
 * with the loss ops listed above.  Algorithmic bytes: n_layers * rows * 12*D (8*D without the gradient). */
int vqa_neg_cos_max_layers(void);
int vqa_neg_cos_rows_multi(const float* const* a, const float* const* b, float* const* ga, int n_layers,
                           float* partial, const uint8_t* row_mask, long mask_period, long rows0, long rows1, int D,
                           long a_stride0, long a_stride1, long b_stride0, long b_stride1, long g_stride0,
                           long g_stride1, float gscale, float cos_eps, float* loss_out, int accumulate,
                           vqa_stream_t stream);

/* dst[0] = (accumulate ? dst[0] : 0) + scale * sum_{i<count} partial[i], summed in index order by one workgroup.
 * Turns the partials of one or more vqa_neg_cos_rows launches into the scalar loss on the device
 * (the reference's float(loss.cpu()) host sync per step, projected_gradient_descent.py:145, is deferred). */
int vqa_sum_partials(const float* partial, int count, float* dst, int accumulate, float scale,
                     vqa_stream_t stream);

/* Masked-LM cross entropy with ignore_index over K label sets, loss and gradient in one launch:
 *   loss = sum_g sum_k mean_{r in group g : labels[k][r] != ignore} ( logsumexp(logits[r,:]) - logits[r, labels[k][r]] )
 * rows_per_group == 0: ONE group = F.cross_entropy's mean over all rows (the reference's op on whatever batch it is
 * given); rows_per_group == L: one group per SAMPLE of a (B*L)-row batch = the batch-1 reference's loss summed over
 * the samples, whose per-sample gradients equal the batch-1 gradients whatever the other samples' labels are.
 * row_loss[r] (scratch, `rows` floats) receives row r's share; loss_out (nullable) receives
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + gscale * sum_r row_loss[r]      (summed in row order, in the launch);
 * grad (nullable, (rows, V) contiguous) receives gscale * d loss / d logits.  labels is int64 [K][rows];
 * scratch holds vqa_ce_scratch_floats(K, groups) floats (the fold's arrival counters + reciprocal valid counts per label
 * set and group; the launch initialises it).  K <= vqa_ce_max_label_sets().
 * A label that is neither ignore_index nor in [0, V) makes the loss NaN and ORs VQA_FLAG_BAD_LABEL into *flag
 * (flag nullable); torch raises a device assert for it, it is never silently ignored.
 * exp() is the hardware exponential (v_exp_f32, ~2 ulp); parity with torch is stated as 1e-4 relative in the tests.
 * The row's logsumexp - logits[r, t] is formed as  log c + log1p(s / c) - (logits[r, t] - m)  with m the row max, c the
 * number of elements equal to it and s the sum of exp(x - m) over the others: a row whose label is predicted with p ~ 1
 * keeps a loss down to 1e-8 accurate to 4e-6 relative, whatever common offset the logits carry (asserted in
 * tests/test_loss_fp64.py).  -inf logits (a masked vocabulary) contribute 0 and get a zero gradient; a row that is
 * entirely -inf, or that holds a NaN anywhere, has a NaN loss, as in torch.
 * Replaces F.cross_entropy(out[0].view(-1, 30522), y[0][...].view(-1), ignore_index=-100), its K-fold repetition for
 * 3-d labels and the autograd backward: A-ch/attacks/fast_gradient_method.py:131-142, V-ch/...:115-126.
 * A row whose K labels are all ignore_index -- every position but the [MASK]-ed answer pieces in the reference's
 * workload, ALBEF_attack/adv_attack.py:433-558 -- has zero loss and a zero gradient whatever its logits are: they are not
 * read and no exponential is evaluated; the row costs its zero gradient store -- or nothing at all:
 * row_state (nullable, `rows` bytes, requires grad): for a caller that hands the SAME gradient buffer to every launch of an
 * attack (zero-filled once, together with row_state, when it is allocated).  row_state[r] != 0 means "the buffer's row r
 * holds a live gradient"; a live row writes its gradient and sets the byte, a dead row stores zeros only if the byte is
 * set and clears it.  With the labels of an attack fixed, dead rows are never written after the allocation.
 * Algorithmic bytes: 8*V per live row (read the logits once from HBM, write the gradient once); per dead row 4*V without
 * row_state, 0 with it. */
int vqa_ce_max_label_sets(void);
long vqa_ce_scratch_floats(int K, long groups);
int vqa_ce_rows(const float* logits, long row_stride, const int64_t* labels, int K, long rows, int V,
                long ignore_index, long rows_per_group, float* scratch, float* grad, float* row_loss, float gscale,
                float* loss_out, int accumulate, int* flag, unsigned char* row_state, vqa_stream_t stream);

/* ---------------------------------------------------------------- text side
 * dst[b, k, :] = src[b, idx[k], :]  for src (B, L, D), idx int64[K] with 0 <= idx[k] < L.
 * Replaces `x[1].grad[:, text_emb_pick]`, A-ch/attacks/fast_gradient_method_vl.py:120 (V-ch: :130). */
int vqa_gather_rows(const float* src, const int64_t* idx, float* dst, int B, int L, int K, int D,
                    vqa_stream_t stream);

/* Candidate-substitution scoring (update_adv_text + dir_sim, ALBEF_attack/adv_attack.py:284-298,325-333;
 * vlmo_module.py:1632-1702).  For candidate c with (sample s, token position p, gradient row k, vocabulary id v):
 *   e   = LayerNorm(word[v] + pos[p] + type[0]; gamma, beta, ln_eps)         (BERT embeddings, position-wise)
 *   d   = e - e_ori[s, p]
 *   out[c] = cos( d / max(|d|, 1e-12),  g / max(|g|, 1e-12) ; eps = 1e-6 ),   g = grad[s, k]
 * cand is int32[n_cand][4] = {s, p, k, v}.  word (V, D), pos (P, D), type (>=1, D), e_ori (S, L, D), grad (S, K, D).
 * D multiple of 4, <= 2048. */
int vqa_cand_dir_sim(const float* word, const float* pos, const float* type, const float* gamma,
                     const float* beta, float ln_eps, const float* e_ori, const float* grad,
                     const int32_t* cand, float* out, int n_cand, int L, int K, int D, vqa_stream_t stream);

/* Masked-token embedding substitution: BERT text embeddings for explicit triples {destination row, token position,
 * vocabulary id}:  dst[row, :] = LayerNorm(word[id] + type[0] + pos[position]; gamma, beta, ln_eps), dst viewed as
 * (rows, D).  With all B*L rows it embeds a question batch in one launch; with a short list it rewrites only the rows
 * of the words the joint attack just substituted.  Replaces the re-tokenise + `text_embeddings(adv_text_ids)` calls
 * between PGD blocks (ALBEF_attack/adv_attack.py:643-645,369-384; models/xbert.py:189-216).
 * triples int32 [n][3]; D multiple of 4, <= 2048; the caller guarantees rows are distinct and in range. */
int vqa_embed_tokens(const float* word, const float* pos, const float* type, const float* gamma, const float* beta,
                     float ln_eps, const int32_t* triples, int n, float* dst, int D, vqa_stream_t stream);

/* Greedy acceptance of the word substitutions of one probe step, for the whole batch, on the device
 * (update_adv_text's sort + acceptance loop, ALBEF_attack/adv_attack.py:299-323; vlmo_module.py:1676-1700), with the
 * bag-of-embeddings stand-in for the reference's TF-Hub sentence encoder (:315-318):
 *   sim(ids) = <m(ori), m(ids)> / (|m(ori)| |m(ids)| + 1e-12),  m(ids) = mean over non-pad (id != 0) tokens of table[id].
 * cand int32 [n][4] = {sample, position, grad row, vocabulary id} (as for vqa_cand_dir_sim); order int32 [n] lists the
 * candidate indices grouped by sample and, within a sample, by descending dir_sim score (stable); seg int32 [B + 1]:
 * order[seg[s] .. seg[s+1]) belong to sample s.  Per sample, in that order: skip a candidate whose position already
 * took a substitution; accept it iff the similarity between the ORIGINAL question and the current question with that
 * position replaced exceeds the threshold, which then rises to that similarity.
 * ori_ids, cur_ids int64 (B, L), L <= 64; cur_ids is updated in place; new_id int32 (B, L) receives the accepted id per
 * position or -1, acc_rank (nullable, int32 (B, L)) the order in which the sample accepted it (0, 1, ...) or -1.
 * table fp32 (V, E), E <= 512.  One wavefront per sample. */
int vqa_greedy_accept(const int32_t* cand, const int32_t* order, const int32_t* seg, int B, int L,
                      const int64_t* ori_ids, int64_t* cur_ids, int32_t* new_id, int32_t* acc_rank, const float* table,
                      int V, int E, float threshold, vqa_stream_t stream);

/* ---------------------------------------------------------------- white-box attention (fp32, head dimension 64)
 * o = softmax(scale * q k^T + bias) v  per (batch, head), exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32),
 * flash-style (the Sq x Sk scores never reach HBM).  The frozen white boxes' `Attention.forward`
 * (vlmo/modules/multiway_transformer.py:88-118; ALBEF_attack/models/vit.py) is a callee of the attack's hot path.
 * q (B, H, Sq, 64), k / v (B, H, Sk, 64), o (B, H, Sq, 64) are addressed through element strides
 * strides[12] = {q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, o_sb, o_ss, o_sh} (batch, sequence, head; the head
 * dimension is dense; all multiples of 4, bases 16-byte aligned) -- q, k, v may be views of one packed qkv tensor.
 * bias (nullable): additive fp32 (relative-position bias and/or -inf key padding), bias_strides[3] = {batch, head, query
 * row} in elements (batch / head stride may be 0, all multiples of 4), key stride 1.  The kernels read bias rows in
 * whole tiles of 32 keys: from every row start, ceil32(Sk) floats must be readable (pad the rows; what lies beyond Sk
 * is masked, never used).  lse (B, H, Sq) receives log-sum-exp of the scores.
 * scores (nullable; vqa_attn_scores_floats(B, H, Sq, Sk) floats, 16-byte aligned): when given, the forward also stores
 * the pre-softmax scores scale * q k^T + bias -- a forward that will be differentiated hands them to vqa_attn_bwd, whose
 * key-block kernel then skips the q k^T product and the bias.  The buffer is OPAQUE: per (batch, head) a grid of 32 x 32
 * tiles over ceil128(Sq) x ceil128(Sk), each tile in the register order of the wave that produced it (csrc/attn.hip);
 * only vqa_attn_bwd of the same B, H, Sq, Sk reads it.
 * key_hole (nullable, int32 (B, 2)): keys [key_hole[2b], key_hole[2b+1]) of batch element b score -inf for every head
 * and query -- the padded text tokens of a question shorter than the batch's text length (key padding of the reference's
 * attention mask).  It lets a ragged batch share ONE (1, H, S, S) relative-position slab (batch stride 0) instead of a
 * per-sample (B, H, S, S) bias.  The stored scores carry the -inf, so the scores-based backward needs nothing else; the
 * score-recomputing forms of vqa_attn_bwd do not know the hole: callers that use them pass the padding inside `bias`.
 * nsplit / split_ws (ABI v4): nsplit == 1 (split_ws ignored) is the form above: one workgroup per (batch, head, 128
 * queries) walks all key tiles.  nsplit > 1 is for SMALL batches -- the reference's own batch 1 gives 12 heads x 5
 * blocks = 60 workgroups for 256 CUs, each a serial chain over ~19 tiles: the key loop is cut into nsplit parts
 * (nsplit <= ceil(Sk / 32)), every part is its own workgroup writing partial accumulators + (running maximum, row sum)
 * into split_ws (vqa_attn_split_ws_floats(B, H, Sq, Sk, nsplit) floats, 16-byte aligned), and a second kernel combines
 * the parts in index order (flash-decoding reduction; deterministic, results equal the unsplit form to fp32 rounding). */
int vqa_attn_fwd(const float* q, const float* k, const float* v, const float* bias, float* o, float* lse, float* scores,
                 int B, int H, int Sq, int Sk, const long* strides, const long* bias_strides, float scale,
                 const int* key_hole, int nsplit, float* split_ws, vqa_stream_t stream);
/* vqa_attn_fwd with its two products on the bf16 matrix pipe: every fp32 operand split exactly into three bf16 planes,
 * a product the six plane products that carry fp32's precision (the arithmetic of vqa_gemm_bf16x6), fp32 accumulation;
 * results are fp32-grade and differ from vqa_attn_fwd's by rounding order.  The same arguments, outputs and `scores`
 * layout (vqa_attn_bwd reads them as it reads vqa_attn_fwd's).  nsplit must be 1 (VQA_ERR_SHAPE otherwise; split_ws is
 * ignored): the loop-split forms are vqa_attn_fwd's.  Meant for a forward that is not differentiated or whose vqa_attn_bwd is
 * given these scores: the score-recomputing forms of vqa_attn_bwd round as vqa_attn_fwd does, and only its lse cancels that.  inf / NaN in q, k, v may come out as NaN.  Additive export: the
 * ABI version stays. */
int vqa_attn_fwd_x6(const float* q, const float* k, const float* v, const float* bias, float* o, float* lse,
                    float* scores, int B, int H, int Sq, int Sk, const long* strides, const long* bias_strides,
                    float scale, const int* key_hole, int nsplit, float* split_ws, vqa_stream_t stream);
long vqa_attn_scores_floats(int B, int H, int Sq, int Sk);
long vqa_attn_split_ws_floats(int B, int H, int Sq, int Sk, int nsplit);

/* Gradients of the above w.r.t. q, k, v given go = d loss / d o (the bias is frozen: no gradient).  Deterministic (no
 * float atomics: bitwise reproducible), two forms:
 *   ds_ws != NULL (vqa_attn_bwd_ws_floats(B, H, Sq, Sk) floats, 16-byte aligned, contents irrelevant): 5 products.  A
 *     streaming pre-pass writes delta (B, H, Sq) = rowsum(go . o); the kernel that owns key blocks computes dk, dv and
 *     stores the dS tiles it forms on the way, transposed, into ds_ws (tiled like `scores`); a third kernel forms dq
 *     from them.  With
 *     scores != NULL (what vqa_attn_fwd stored for the same operands) the key-block kernel reads the scores instead of
 *     recomputing them: 4 products.
 *   ds_ws == NULL: 7 products, no workspace: one kernel owns query blocks (dq; it also writes delta), one owns key
 *     blocks (dk, dv); both recompute the probabilities from lse.
 * grad_strides[12] = {go_sb, go_ss, go_sh, dq_sb, dq_ss, dq_sh, dk_sb, dk_ss, dk_sh, dv_sb, dv_ss, dv_sh} (elements;
 * dq / dk / dv may be the three slices of one packed (B, S, 3, H, 64) gradient buffer).
 * nsplit / split_ws (ABI v4; needs ds_ws and scores): as in vqa_attn_fwd -- the key-block kernel's loop over query
 * tiles and the dq kernel's loop over key tiles are cut into nsplit parts (nsplit <= min(ceil(Sq / 32), ceil(Sk / 32)))
 * whose partial dk / dv / dq are summed in part order by a small kernel (the same split_ws serves both, in turn). */
int vqa_attn_bwd(const float* q, const float* k, const float* v, const float* bias, const float* o, const float* go,
                 const float* lse, const float* scores, float* delta, float* dq, float* dk, float* dv, float* ds_ws, int B,
                 int H, int Sq, int Sk, const long* strides, const long* bias_strides, const long* grad_strides,
                 float scale, int nsplit, float* split_ws, vqa_stream_t stream);
/* The saved-scores form of vqa_attn_bwd (scores != NULL, ds_ws != NULL, nsplit == 1) with the three products of its
 * key-block kernel -- dP = go . v^T, dv = P^T . go, dk = dS^T . q -- on the bf16 matrix pipe as six exact bf16 plane
 * products each (the arithmetic of vqa_attn_fwd_x6); the delta pre-pass, the dS^T workspace and the dq kernel are
 * vqa_attn_bwd's.  Same arguments; results are fp32-grade and differ from vqa_attn_bwd's by rounding order.  Returns
 * VQA_ERR_SHAPE and launches nothing unless scores, ds_ws and nsplit == 1 are all given: every other form is
 * vqa_attn_bwd's (and so is a q or go whose sequence stride is negative or 2^24 elements and more).  `scores` may come
 * from either forward.  inf / NaN in go, q, v may come out as NaN.  Additive export:
 * the ABI version stays. */
int vqa_attn_bwd_x6(const float* q, const float* k, const float* v, const float* bias, const float* o, const float* go,
                    const float* lse, const float* scores, float* delta, float* dq, float* dk, float* dv, float* ds_ws,
                    int B, int H, int Sq, int Sk, const long* strides, const long* bias_strides, const long* grad_strides,
                    float scale, int nsplit, float* split_ws, vqa_stream_t stream);
long vqa_attn_bwd_ws_floats(int B, int H, int Sq, int Sk);

/* ---------------------------------------------------------------- input pipeline
 * Pillow-exact bicubic resize of an 8-bit interleaved image (H, W, C), C <= 4, then ToTensor + Normalize into planar
 * fp32 -- what `transforms.Resize((res, res), interpolation=Image.BICUBIC)`, `ToTensor()`, `Normalize(0.5, 0.5)` do on
 * the host in the reference (ALBEF_attack/dataset/__init__.py:17,35-39; vlmo/transforms/square_transform.py:11-18).
 * kk int32 [out][ksize] fixed-point taps (22 fractional bits) and bounds int32 [out][2] = {first source index, tap
 * count} are Pillow's precompute_coeffs + normalize_coeffs_8bpc tables (vqattack_amd/preprocess.py builds them).
 *   pass 1: dst[y, xo, c] uint8 (H, W_out, C)         = horizontal resampling of src
 *   pass 2: dst[c, yo, x] fp32  (C, H_out, W)          = (vertical resampling of src / 255 - mean) / std
 *           (kk == NULL: no vertical resampling, requires H_in == H_out -- conversion only)
 * dst of pass 2 is typically `batch + b*3*S*S`, the image's slot of the attack's (B, 3, S, S) tensor. */
int vqa_resize_bicubic_h_u8(const uint8_t* src, int h, int w_in, int c, const int32_t* kk, const int32_t* bounds,
                            int ksize, int w_out, uint8_t* dst, vqa_stream_t stream);
int vqa_resize_bicubic_v_normalize(const uint8_t* src, int h_in, int w, int c, const int32_t* kk,
                                   const int32_t* bounds, int ksize, int h_out, float mean, float stdv, float* dst,
                                   vqa_stream_t stream);

/* ---------------------------------------------------------------- white-box block glue (callee of the hot path)
 * The frozen encoders' pre-LN transformer block -- reference: VLMO_VQAttack/vlmo/modules/multiway_transformer.py:184-201
 * (x = x + gamma_1 * attn(norm1(x)); text tokens through norm2_text / mlp_text, image tokens through norm2_imag /
 * mlp_imag, split at max_text_len :193-197; x = x + gamma_2 * mlp) and ALBEF's ViT block (ALBEF_attack/models/vit.py) --
 * executed without an autograd graph by vqattack_amd/whitebox/_fused.py: library GEMMs + vqa_attn_* + these four entry
 * points.  Rows are D contiguous floats (D % 4 == 0, D <= 1024), every pointer 16-byte aligned.
 * Token layout for the modality split: a batch element has `period` rows (tokens), the first `split` are text tokens
 * (segment 0), the rest image tokens (segment 1); a "split" tensor is two contiguous buffers, (B*split, D) and
 * (B*(period-split), D) -- what the two expert GEMMs read and write.  period == 0: no split anywhere.
 *
 * vqa_ln_fwd: optional prologue  x_out = x + rscale * r  (r0 != NULL; r given whole as r0, or split as r0 / r1;
 *   rscale NULL = 1), then  y = LayerNorm(x_out; gamma, beta, eps)  with (gamma1, beta1) for segment-1 rows when given,
 *   y written whole (y1 == NULL) or split (y0 / y1); mean[row], rstd[row] saved for the backward.  The statistics are
 *   taken on the row centred on its first element, so rows far from zero or nearly constant keep their spread; the
 *   backward reads rstd and forms x - mean from x in the same way (bitwise what the forward used).  Without a prologue
 *   x_out is not written; with one, x_out may be NULL (a forward-only caller that never reads the sum: 12 B/element).
 *   16 B/element with prologue, 8 without.  Replaces torch.addcmul + torch.cat + two slice copies
 *   + F.layer_norm per stage (multiway_transformer.py:186-199).
 * vqa_ln_bwd: dx = (g_a ? g_a : 0) + (g_inj ? g_inj : 0) + dLayerNorm/dx(dy; x, mean, rstd, gamma)  (frozen gamma/beta:
 *   input gradient only); dy whole (dy1 == NULL) or split; g_a = gradient arriving over the residual path, g_inj = the
 *   loss kernel's gradient of this feature map (vqa_neg_cos_rows_multi's ga[layer]); and, when dr0 != NULL,
 *   dr = rscale * dx (rscale NULL = 1) written whole or split (dr1): the gradient of the branch the forward prologue
 *   added.  20-28 B/element.  Replaces layer_norm's backward, the gradient-accumulation adds, addcmul's backward and the
 *   slice / cat backward copies.
 * vqa_ln_bwd_post: the same stage of a POST-LN block  y = LayerNorm(s),  s = x + f(x)  -- the BERT fusion encoder of
 *   ALBEF, reference ALBEF_attack/models/xbert.py BertSelfOutput.forward / BertOutput.forward
 *   (hidden_states = self.LayerNorm(hidden_states + input_tensor)), forward by vqa_ln_fwd with r0 / x_out (x_out = s):
 *   ds = dLayerNorm/dx((dy_a + (dy_b ? dy_b : 0)) + (g_inj ? g_inj : 0); s, rstd, gamma)  -- the gradients that reach y
 *   (at most three in a BERT layer: the next layer's residual path, the input gradient of its packed q/k/v projection,
 *   the loss kernel's gradient of this feature map) are summed in that fixed order BEFORE the LayerNorm backward, which
 *   vqa_ln_bwd (sum after) cannot express.  ds is the gradient of x over the residual path AND of the branch f(x); it is
 *   written once.  The LayerNorm arithmetic is vqa_ln_bwd's: with dy_b == g_inj == NULL the result has the bits of
 *   vqa_ln_bwd(dy_a, ...) without g_a / g_inj.  12-20 B/element.  Replaces layer_norm's backward, the add's backward and
 *   the gradient-accumulation adds.
 * vqa_gelu_fwd / vqa_gelu_bwd: a = gelu(h) / dh = da * gelu'(h), exact erf form (nn.GELU() of the reference's Mlp,
 *   multiway_transformer.py:36-55); dh may alias da. */
int vqa_ln_fwd(const float* x, const float* r0, const float* r1, const float* rscale, float* x_out,
               const float* gamma0, const float* beta0, const float* gamma1, const float* beta1, float* y0, float* y1,
               float* mean, float* rstd, long rows, int D, long period, long split, float eps, vqa_stream_t stream);
int vqa_ln_bwd(const float* dy0, const float* dy1, const float* x, const float* mean, const float* rstd,
               const float* gamma0, const float* gamma1, const float* g_a, const float* g_inj, const float* rscale,
               float* dx, float* dr0, float* dr1, long rows, int D, long period, long split, vqa_stream_t stream);
int vqa_ln_bwd_post(const float* dy_a, const float* dy_b, const float* g_inj, const float* s, const float* rstd,
                    const float* gamma, float* ds, long rows, int D, vqa_stream_t stream);
int vqa_gelu_fwd(const float* h, float* a, size_t n, vqa_stream_t stream);
int vqa_gelu_bwd(const float* h, const float* da, float* dh, size_t n, vqa_stream_t stream);

/* ---------------------------------------------------------------- encoder GEMMs on the bf16 matrix pipe (csrc/gemm.hip)
 * C[M, N] = A[M, K] . B (+ bias[N])  with A fp32 (row stride lda, lda % 4 == 0, 16-byte aligned), C fp32 (row stride
 * ldc) and B a frozen weight packed once into three bf16 planes (b = b0 + b1 + b2, exact): the six products a0b0, a0b1,
 * a1b0, a0b2, a1b1, a2b0 run on v_mfma_f32_16x16x32_bf16 with A split the same way on the fly ("bf16x6"); error at or
 * below the fp32 GEMM's.  N % 128 == 0, K % 32 == 0, any M >= 0.  Deterministic (fixed order, no atomics).
 * vqa_gemm_packed_bytes: bytes of a packed [K, N] operand (0 = unsupported shape).
 * vqa_gemm_pack_b: packed <- B[k][n] = trans ? w[n * ldw + k] : w[k * ldw + n]  -- trans = 1 packs the forward operand
 *   W^T of a Linear weight W [out, in] (K = in, N = out), trans = 0 the input-gradient operand W (K = out, N = in).
 *   Layout: bf16 [K/32][N/16][plane 3][lane 64][8], element (k, n) at lane (n % 16) + 16 * ((k % 32) / 8), slot k % 8. */
size_t vqa_gemm_packed_bytes(int K, int N);
int vqa_gemm_pack_b(const float* w, long ldw, int trans, void* packed, int K, int N, vqa_stream_t stream);
int vqa_gemm_bf16x6(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M, int N,
                    int K, vqa_stream_t stream);

/* vqa_gemm_bf16x6_tile: vqa_gemm_bf16x6 with the output tile of a workgroup chosen by the caller; argument rules and
 *   return codes of vqa_gemm_bf16x6, any other tile value VQA_ERR_SHAPE.  VQA_GEMM_TILE_256X128 is vqa_gemm_bf16x6
 *   itself.  VQA_GEMM_TILE_128X256 splits half as much of A per product (every A value is split by N / 256 workgroups
 *   instead of N / 128) and needs N % 256 == 0; for every other N it runs the 256 x 128 tile.  Same packed operand, same
 *   product and k-step order: both tiles give every output the same bits. */
#define VQA_GEMM_TILE_256X128 0
#define VQA_GEMM_TILE_128X256 1
int vqa_gemm_bf16x6_tile(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, int tile, vqa_stream_t stream);

/* vqa_gemm_bf16x6_persistent: the 128 x 256 tile of vqa_gemm_bf16x6_tile as ONE launch of `workgroups` workgroups that
 *   each walk a fixed list of tiles (blockIdx arithmetic: no atomics, no counters, nothing to reset between launches, so
 *   the launch may be captured and replayed).  A tile's last k-step stages the first k-step of the workgroup's next
 *   tile, so only a workgroup's first tile waits for its operands with the matrix pipe idle.  Every output has the bits
 *   of vqa_gemm_bf16x6_tile.  Argument rules and return codes of vqa_gemm_bf16x6_tile with VQA_GEMM_TILE_128X256, except
 *   that N % 256 != 0 is VQA_ERR_SHAPE (there is no other tile to run).  workgroups: at least 1, else VQA_ERR_SHAPE;
 *   one per compute unit is the intended value, and a value above the tile count ceil(M / 128) * (N / 256) is clamped to
 *   it.  A refused call launches nothing.  Never allocates, never synchronises. */
int vqa_gemm_bf16x6_persistent(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                               int N, int K, int workgroups, vqa_stream_t stream);

/* vqa_gemm_bf16x6_half: vqa_gemm_bf16x6 on 128 x 128 output tiles (half a large tile's k-loop work per workgroup, one
 *   workgroup per CU like them); argument rules and return codes of vqa_gemm_bf16x6, the same bits.
 * vqa_gemm_bf16x6_tail: one product in two launches, back to back on `stream`: rows [0, m_split) on `tile` as
 *   vqa_gemm_bf16x6_tile runs them, rows [m_split, M) on the 128 x 128 tile.  The large tiles run in rounds of one
 *   workgroup per CU and the last round takes as long as a full one; with m_split at the end of the last full round
 *   (ops.gemm_tail_plan) the remaining rows run as twice as many workgroups of half the length.  Every output has the
 *   bits vqa_gemm_bf16x6_tile gives it.  Argument rules and return codes of vqa_gemm_bf16x6_tile; 0 <= m_split <= M, else
 *   VQA_ERR_SHAPE.  m_split == M is vqa_gemm_bf16x6_tile itself, m_split == 0 vqa_gemm_bf16x6_half itself.  A refused call
 *   launches nothing.  Never allocates, never synchronises. */
int vqa_gemm_bf16x6_half(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, vqa_stream_t stream);
int vqa_gemm_bf16x6_tail(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                         int N, int K, int tile, long m_split, vqa_stream_t stream);

/* vqa_gemm_bf16x6_small: the same product from the same packed operand on 64 x 128 output tiles, for row counts whose
 *   256 x 128 tiles cannot fill the device, with an optional deterministic split over K.  Argument rules and return
 *   codes of vqa_gemm_bf16x6; 1 <= ksplit <= min(K / 32, 16), else VQA_ERR_SHAPE.  With nk = K / 32 k-steps, part p covers
 *   the k-steps [p * nk / ksplit, (p + 1) * nk / ksplit) (integer division).  ksplit == 1: C = acc + bias with the bits of
 *   vqa_gemm_bf16x6; ws is not touched and may be NULL.  ksplit > 1: every part stores its fp32 partial product P_p to
 *   ws ([ksplit][M][N] floats, 16-byte aligned, vqa_gemm_small_ws_bytes; NULL -> VQA_ERR_NULL) and a second kernel on
 *   the same stream forms C = ((P_0 + P_1) + ... + P_(ksplit-1)) + bias, in that order, in fp32.  No atomics and no
 *   counters: bitwise reproducible, nothing to reset between launches.  Never allocates, never synchronises.
 * vqa_gemm_small_ws_bytes: bytes of that workspace; 0 when ksplit == 1 or the shape is unsupported. */
size_t vqa_gemm_small_ws_bytes(long M, int N, int ksplit);
int vqa_gemm_bf16x6_small(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                          int N, int K, int ksplit, void* ws, vqa_stream_t stream);

/* vqa_gemm_bf16x6_epi: vqa_gemm_bf16x6_tile with the FFN's GELU, or the product with its derivative, applied to the
 *   accumulators in the GEMM's epilogue -- the activation of the reference's Mlp.forward (x = self.act(self.fc1(x)),
 *   VLMO_VQAttack/vlmo/modules/multiway_transformer.py:36-55; ALBEF_attack/models/vit.py Mlp) and of BertIntermediate
 *   (ALBEF_attack/models/xbert.py: intermediate_act_fn(dense(hidden_states))) without the pass over the pre-activation
 *   that vqa_gelu_fwd / vqa_gelu_bwd make.  Same prologue, k-loop, packed operand and product order as the unfused
 *   kernels; the GELU arithmetic is vqa_gelu_fwd's / vqa_gelu_bwd's, so every output has the bits of the two-step form.
 *   VQA_GEMM_EPI_NONE: vqa_gemm_bf16x6_tile itself (aux, ldaux ignored).
 *   VQA_GEMM_EPI_GELU: h = acc (+ bias);  aux[row * ldaux + col] = h where aux != NULL;  C = gelu(h).
 *   VQA_GEMM_EPI_GELU_GRAD: C = (acc (+ bias)) * gelu'(aux[row * ldaux + col]);  aux (the forward's h, read only) is
 *     required: NULL -> VQA_ERR_NULL.
 *   Argument rules and return codes of vqa_gemm_bf16x6_tile (VQA_GEMM_TILE_128X256 with N % 256 != 0 runs the fused
 *   256 x 128 kernel), and: any other epilogue VQA_ERR_SHAPE; aux given with ldaux < N VQA_ERR_SHAPE; aux not 4-byte
 *   aligned VQA_ERR_ALIGN; M == 0 VQA_OK.  aux must not overlap C or A: rows >= M of aux are neither read nor written,
 *   but nothing orders one workgroup's stores against another's loads.  Only pointer equality is detected: aux == C
 *   or aux == A returns VQA_ERR_SHAPE (a return code of this entry point alone; vqa_gemm_bf16x6_tile has no such
 *   operand).  Never allocates, never synchronises. */
#define VQA_GEMM_EPI_NONE 0
#define VQA_GEMM_EPI_GELU 1
#define VQA_GEMM_EPI_GELU_GRAD 2
int vqa_gemm_bf16x6_epi(const float* A, long lda, const void* packed, const float* bias, float* C, long ldc, long M,
                        int N, int K, int tile, int epilogue, float* aux, long ldaux, vqa_stream_t stream);

/* vqa_gemm_bf16x6_grouped: up to VQA_GEMM_MAX_GROUPS products with one (N, K) -- group i is
 *   C[i] = epilogue(A[i] . packed[i] (+ bias[i])) on M[i] rows -- as ONE launch of 128 x 256 tiles: the expert FFNs of a
 *   multiway block (text and image rows through different weights, VLMO_VQAttack/vlmo/modules/multiway_transformer.py:
 *   193-197), where the small expert's tiles ride in the last, partly empty round of the large one's instead of a launch
 *   that cannot fill the device.  The tile list is group 0's row blocks, then group 1's, ...; a workgroup finds its
 *   group from its row block.  Prologue, k-loop and epilogues are those of vqa_gemm_bf16x6_epi on
 *   VQA_GEMM_TILE_128X256: every output of group i has the bits of that call on group i alone.
 *   A, lda, packed, bias, C, ldc, aux, ldaux, M are HOST arrays of n_groups entries, read during the call and copied into
 *   the kernel arguments (no device-side table: capture-safe).  `bias` may be NULL (no group has one) and so may any
 *   bias[i]; `aux` / `ldaux` may be NULL where no group has an aux; with VQA_GEMM_EPI_NONE aux and ldaux are ignored.
 *   1 <= n_groups <= VQA_GEMM_MAX_GROUPS, N % 256 == 0, K % 32 == 0, every M[i] >= 0, at most 2^31 - 1 tiles in all, an
 *   epilogue of vqa_gemm_bf16x6_epi: else VQA_ERR_SHAPE.  A group with M[i] == 0 contributes nothing and its other
 *   entries are not looked at; every group with rows obeys the argument rules of vqa_gemm_bf16x6_epi and gets its return
 *   codes (aux[i] required for VQA_GEMM_EPI_GELU_GRAD; aux[i] == C[i] or A[i] VQA_ERR_SHAPE; a NULL table VQA_ERR_NULL).
 *   Every group is checked ahead of the launch: a refused call leaves every C untouched.  All M[i] == 0: VQA_OK, no
 *   launch.  The 16-byte epilogue runs only where every group with rows qualifies for it, the dword form otherwise (same
 *   bits).  The output (and aux) ranges of different groups must not overlap each other or any group's A or aux: that
 *   is the caller's duty, nothing here detects it.  Never allocates, never synchronises. */
#define VQA_GEMM_MAX_GROUPS 4
int vqa_gemm_bf16x6_grouped(const float* const* A, const long* lda, const void* const* packed, const float* const* bias,
                            float* const* C, const long* ldc, float* const* aux, const long* ldaux, const long* M,
                            int n_groups, int N, int K, int epilogue, vqa_stream_t stream);

/* vqa_gemm_bf16x6_lse: the cross entropy of an LM head without its logits -- row_loss[row] = logsumexp_c(x[row, c]) -
 *   x[row, targets[row]] over c < n_valid, with x = A . B + bias the product vqa_gemm_bf16x6_tile would have stored.
 *   It replaces the vocabulary logits and F.cross_entropy(reduction='none') of the reference's answer ranking
 *   (ALBEF_attack/models/model_vqa.py:149-203 with the LM loss of ALBEF_attack/models/xbert.py:1265-1271), which
 *   materialise [rows, vocabulary] twice to obtain one number per row.
 *   The same prologue, k-loop, packed operand and product order as vqa_gemm_bf16x6_epi, with a third epilogue
 *   (VQA_GEMM_EPI_LSE of csrc/gemm.hip; it has operands of its own, so it is no value of vqa_gemm_bf16x6_epi's
 *   `epilogue` and is not defined here): no C is stored.  Every
 *   wave reduces its 64 x 64 block of x, columns >= n_valid masked to -inf, to one (max, sum exp(x - max)) pair per row
 *   and stores it to ws; the lane that holds column targets[row] stores that x (the bits of C[row, target]).  A second
 *   kernel on the same stream folds a row's N / 64 pairs in block order and writes
 *     lse[row] (nullable) = max + log(sum);
 *     row_loss[row] = lse - x[row, target];  exactly 0 where targets[row] == ignore_index;  NaN, with
 *     VQA_FLAG_BAD_LABEL ORed into *flag (nullable), where it is neither ignore_index nor in [0, n_valid).
 *   exp is the hardware v_exp_f32, as in vqa_ce_rows: 1e-4 relative against torch.  No atomics on the values, fixed
 *   order: bitwise reproducible, and both tiles give the same bits (a wave's block is 64 x 64 in both).  A NaN in a row
 *   of A makes that row NaN and no other; a block of 64 columns that is all -inf or all padding contributes (-inf, 0).
 *   B is packed from a weight padded to N columns (what the pad columns hold does not matter: they are masked);
 *   bias (nullable) has N entries.  N % 128 == 0, K % 32 == 0, 0 < n_valid <= N, else VQA_ERR_SHAPE; lda rules and
 *   the tile argument of vqa_gemm_bf16x6_tile.  ws: vqa_gemm_lse_ws_floats(M, N) floats, 16-byte aligned (else
 *   VQA_ERR_ALIGN): [N / 64][M] pairs, then the M target logits.  targets: int64 [M].  M == 0 VQA_OK.  Never
 *   allocates, never synchronises.
 * vqa_gemm_lse_ws_floats: floats of that workspace; 0 for an unsupported shape. */
long vqa_gemm_lse_ws_floats(long M, int N);
int vqa_gemm_bf16x6_lse(const float* A, long lda, const void* packed, const float* bias, long M, int N, int K,
                        int n_valid, const int64_t* targets, long ignore_index, float* ws, float* row_loss, float* lse,
                        int* flag, int tile, vqa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VQATTACK_HIP_H */
