/*
 * pcd_hip.h -- C ABI of the MI355X (gfx950) point-cloud diffusion sampler library.
 *
 * The reference (dhillon24/3d-shape-generation) has no FFI/plugin layer: its
 * boundary is the Python object API of diffusion.py / networks.py / metrics.py
 * (SURVEY.md section 8(b)).  This header is the C-ABI shared-library boundary
 * that sits UNDER a re-implementation of that Python API; each entry point
 * cites the reference code it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - the caller owns all memory; nothing is retained except by *_create handles,
 *    which keep the pointers given in their descriptor (they must outlive the handle);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued, never synchronised;
 *  - return value: 0 = ok, negative = error, message via pcd_last_error() (thread local);
 *  - activations are point-major: row m = b*N + n holds the C channels of point n
 *    of shape b, fp16 ("f16") unless stated; weights are [C_out][K] fp16 row-major
 *    (the reference's Conv1d (C_out, C_in, 1) / Linear (out, in) layout, K contiguous).
 */
#ifndef PCD_HIP_H
#define PCD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCD_OK 0
#define PCD_ERR_ARG (-1)
#define PCD_ERR_HIP (-2)
#define PCD_ERR_WORKSPACE (-3)

/* The ABI version this header describes: bumped whenever a signature or a descriptor struct changes (2: pcd_latent_persist_status takes the
 * launch stream; the descriptor structs pcd_unet_desc_t / pcd_sab_desc_t / pcd_conv3d_desc_t / the VAE residual descriptor as they stand since round 4).
 * A binding compares pcd_abi_version() of the library it loaded with the PCD_ABI_VERSION it was written against and refuses a mismatch. */
#define PCD_ABI_VERSION 2

const char* pcd_last_error(void);
/* the PCD_ABI_VERSION the library was built from */
int pcd_abi_version(void);
/* 0 if a gfx950 device is usable by this process, negative otherwise */
int pcd_device_check(void);

/* ------------------------------------------------------------------ GEMM (K1)
 * out[m][c] = act( sum_k A[m][k] * W[c][k] + bias[c] + shape_bias[m / rows_per_shape][c] )
 * Replaces every Conv1d(k=1)+BatchNorm1d(eval)+ReLU of networks.py:46-48 (BN folded
 * into W,bias by the host) and the Linear layers of networks.py:64-66.
 * A may be the K-concatenation of two sources [A1 (K1 cols) | A2 (K2 cols)]
 * (the torch.cat skip inputs of networks.py:811-814) without materialising it.
 * K1, K2 multiples of 64; C multiple of 8.
 */
typedef struct {
    const void* a1; int64_t lda1; int k1;      /* fp16 [M][lda1] */
    const void* a2; int64_t lda2; int k2;      /* optional second source, NULL/0 */
    const void* w;  int64_t ldw;               /* fp16 [C][ldw], ldw >= k1+k2 */
    const float* bias;                         /* fp32 [C] or NULL */
    const float* shape_bias; int rows_per_shape; /* fp32 [ceil(M/rows_per_shape)][C] or NULL */
    int relu;                                  /* 1: max(.,0) */
    int m, c;
} pcd_gemm_desc_t;

/* epilogue: store fp16 out[m][ldo] */
int pcd_gemm_f16(const pcd_gemm_desc_t* d, void* out, int64_t ldo, void* stream);
/* the same with hi / lo weights: w is [c][2 (k1 + k2)] (ldw >= that): columns [0, K) the fp16 weights, [K, 2K) the fp16 of their
 * rounding residuals; the sources are walked twice (all hi products, then all lo products, fp32 accumulation): ~22-bit weights */
int pcd_gemm_f16_hilo(const pcd_gemm_desc_t* d, void* out, int64_t ldo, void* stream);
/* epilogue: store fp32 out[m][ldo] */
int pcd_gemm_f16_out32(const pcd_gemm_desc_t* d, float* out, int64_t ldo, void* stream);
/* split-K form for short-and-wide products with a long reduction (the backward-weight products dW = dz^T a of the
 * training step, reduction over the B*N points): slabs[s][m][c] = A[:, s*K/S:(s+1)*K/S] W[:, same]^T, fp32, all S
 * slices in ONE launch (S * tiles of work instead of a handful).  k2 = 0, no bias/relu; K/S a multiple of 64.
 * pcd_sum_slabs_f32 then adds the S slabs in a fixed order into out[rows][ldo] (deterministic, no float atomics). */
int pcd_gemm_f16_splitk(const pcd_gemm_desc_t* d, int splits, float* slabs, void* stream);
int pcd_sum_slabs_f32(const float* slabs, int nslabs, int64_t rows, int cols, float* out, int64_t ldo, void* stream);
/* epilogue: residual add, out[m][c] = resid[m][c] + (A W^T + bias), fp16 in/out (networks.py:81-82) */
int pcd_gemm_f16_residual(const pcd_gemm_desc_t* d, const void* resid, int64_t ldr,
                          void* out, int64_t ldo, void* stream);
/* epilogue: per-shape column max, colmax[s][c] = max over the rows of shape s (post-ReLU,
 * so values >= 0); replaces torch.max(global_feat, 2) of networks.py:807 without ever
 * writing the (B,4096,N) tensor.  colmax fp32 [n_shapes][C] must be zeroed by the caller
 * (pcd_fill_zero) before the call; requires d->relu == 1. */
int pcd_gemm_f16_colmax(const pcd_gemm_desc_t* d, float* colmax, int rows_per_shape, void* stream);

/* the column-max GEMM with the weights in MFMA-fragment order, read straight from global memory into the MFMA operand registers (csrc/gemm_f16.hip:
 * gemm_xw_kernel; only the activation panel goes through LDS): wfrag = pcd_gemm_pack_wfrag's copy of w ([c][ldw], k = k1 + k2 columns used, c % 256 == 0,
 * same byte count as the k x c weights).  Whole 256 x 256 tiles, at least 256 of them and a multiple of 256; bias required; no per-shape bias. */
int pcd_gemm_pack_wfrag(const void* w, int64_t ldw, int k, int c, void* wfrag, void* stream);
int pcd_gemm_f16_colmax_wfrag(const pcd_gemm_desc_t* d, const void* wfrag, float* colmax, int rows_per_shape, void* stream);
/* 1 unless pcd_gemm_set_config(8) switched the fragment-order path off (9: on): callers that hold a copy ask before they use it */
int pcd_gemm_wfrag_enabled(void);
/* pcd_gemm_f16 (bias [+ per-shape bias] [+ ReLU], fp16 store) for a caller that holds wfrag = pcd_gemm_pack_wfrag's copy of d->w: where the launch shape
 * allows (whole 256 x 256 tiles, a multiple of 256 of them, k1 + k2 >= 384, one A layout) gemm_xs_kernel runs -- weights straight from global memory,
 * and most of each output tile leaves through LDS DURING the next tile's K loop instead of as one store burst behind it; otherwise pcd_gemm_f16's
 * kernels run.  Bitwise the same output either way.  pcd_gemm_set_config(10) / (11): that kernel off / on (default on); pcd_gemm_store_wfrag_enabled reads it. */
int pcd_gemm_f16_wfrag(const pcd_gemm_desc_t* d, const void* wfrag, void* out, int64_t ldo, void* stream);
int pcd_gemm_store_wfrag_enabled(void);
/* diagnostic (dev tools): the following pcd_gemm_f16_colmax_wfrag launches write, per workgroup, (shader-clock cycles, 100-MHz ticks) of its whole tile walk to
 * stamps[256][2] (uint64, device memory); NULL switches it off.  In-kernel clock = cycles / ticks x 100 MHz (MI355X_MICROARCH.md, DVFS item 6). */
int pcd_gemm_wfrag_stamps(void* stamps);
/* Which of the GEMM kernels run: one code sets one field of the process's GEMM configuration (csrc/gemm_f16.hip: GemmConfig) and leaves the others.
 * TEST / BENCHMARK ONLY: process-global, read by every handle at every launch -- not for use while another thread is launching.
 * PCD_ERR_ARG unless -1 <= code <= 31, code == 33 or 35 <= code <= 38.
 *
 *   code       field            effect
 *   -1         tile             (default) the shape heuristic picks the generic tile
 *   0 .. 4     tile             every following launch uses 0: 128x64, 1: 128x128, 2: 256x128 3-stage, 3: 256x256, 4: 128x128 3-stage
 *   5 / 7 / 6  xp_depth         the 256x256 store / column-max / residual kernel that requests the next tile's first K tile(s) before the epilogue's
 *                               stores (gemm_xp_kernel, whole tiles only): off / one K tile ahead (default) / two (store epilogue only; the others stay at one)
 *   8 / 9      xw               pcd_gemm_wfrag_enabled() off / on (default): read by callers that hold a fragment-order copy, not by pcd_gemm_f16_colmax_wfrag
 *   10 / 11    xs               pcd_gemm_f16_wfrag runs gemm_xs_kernel: off / on (default); pcd_gemm_store_wfrag_enabled() reads it
 *   12 / 13    request_pos      the fragment-order kernels (gemm_xw_kernel, gemm_xs_kernel) request a K tile's LDS-DMA pieces at its top (default) / behind its
 *                               first 32 MFMAs (measured: 14 % slower; kept as the experiment that shows the K loop waits on those pieces).  Same bits.
 *   14 / 15    split_requests   those pieces are requested by every wave (4 each) / by one wave per SIMD (8 each, default).  Same bits.
 *   16 + bits  xs_ablation      timing ablations of gemm_xs_kernel (1: no direct stores, 2: no drip; 16 clears).  OUTPUTS WRONG while set.
 *   33         request_pos = 2  diagnostic: gemm_xw_kernel reloads k step 0's weights late.  The store kernel has no such form: while this is set,
 *                               gemm_xs_kernel runs its request_pos = 1 instance (the one of code 13).  Outputs not promised; 12 clears.
 *   35/36/37   xs_ablation      = 16 / 32 / 48: the ablation instance sends its drip stores out in the direct stores' shape (16: 16 rows x 64 bytes, half
 *                               lines) / its direct stores in the drip's (32: 8 rows x 128 bytes, whole lines), to the wrong places of the same output
 *                               tile (profiles/gemm_store_lines.md).  OUTPUTS WRONG while set; 16 clears.
 *   38         xs_ablation      = 64: the ablation instance with nothing ablated (the control of 35 .. 37; outputs right).  16 clears. */
int pcd_gemm_set_config(int cfg);
/* What a GEMM entry point would launch for `d` under the current configuration, without launching and without touching a device (csrc/gemm_f16.hip:
 * plan_gemm, the function the entry points themselves launch from).  TESTS AND TOOLS ONLY -- no product code needs it.  `entry` names the entry
 * point; rows_per_shape is the column-max entries' argument, splits pcd_gemm_f16_splitk's (both ignored elsewhere), has_wfrag whether a fragment-order
 * copy would be passed.  The descriptor's pointers are compared with NULL and never read.  PCD_ERR_ARG where the entry point would refuse. */
enum { PCD_GEMM_ENTRY_F16 = 0, PCD_GEMM_ENTRY_HILO, PCD_GEMM_ENTRY_OUT32, PCD_GEMM_ENTRY_SPLITK, PCD_GEMM_ENTRY_RESIDUAL, PCD_GEMM_ENTRY_COLMAX,
       PCD_GEMM_ENTRY_COLMAX_WFRAG, PCD_GEMM_ENTRY_WFRAG };
enum { PCD_GEMM_FAMILY_XP = 5, PCD_GEMM_FAMILY_XW = 6, PCD_GEMM_FAMILY_XS = 7 };   /* 0 .. 4: gemm_f16_kernel at that tile */
typedef struct {
    int family;                      /* 0 .. 4 or PCD_GEMM_FAMILY_*: gemm_xp_kernel, gemm_xw_kernel, gemm_xs_kernel */
    int instance;                    /* xw: 0 default, 1 every wave requests, 2 requests behind k step 0, 3 late weights.  xs: 4 * (R - 1) + the same 0, 1, 2,
                                      * or 3 = the ablation instance (R = 1: 12 or more K tiles, parked output chunks leave one per K tile; R = 2: two).  Else 0 */
    unsigned grid, block;
    int tiles_m, tiles_n;
    int patch_pn, patch_xn;          /* XCD patch map: column tiles per patch, XCDs per patch row; 0, 0 = linear tile order */
    int xp_depth;                    /* gemm_xp_kernel: K tiles of the next tile requested ahead (1 or 2), else 0 */
    int xs_ablation;                 /* gemm_xs_kernel's ablation instance: the bits, else 0 */
    int zero_bias, zero_shape_bias;  /* the launch puts the library's row of zeros in place of the missing bias / per-shape bias */
    int no_zero_row;                 /* if that row cannot be had (stream capture before the first eager call, or c > 16384): 0 the generic kernel of the
                                      * same tile runs, 1 pcd_gemm_f16's choice runs, 2 the entry point returns PCD_ERR_ARG */
} pcd_gemm_plan_t;
int pcd_gemm_plan(const pcd_gemm_desc_t* d, int entry, int rows_per_shape, int splits, int has_wfrag, pcd_gemm_plan_t* plan);

int pcd_fill_zero(void* p, size_t bytes, void* stream);
int pcd_f32_to_f16(const float* src, void* dst, int64_t n, void* stream);
int pcd_f16_to_f32(const void* src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------- time embedding + enc1 (K3)
 * For each of n_t time values: sinusoidal embedding (networks.py:820-838, freqs
 * passed in, computed on the host with the reference's torch ops) -> time_mlp
 * Linear/SiLU/Linear (networks.py:737-741) -> temb[n_t][dim].
 * If e1w_t != NULL also the hoisted time half of enc1.conv1:
 * tbias[i][c] = sum_j e1w_t[c][j]*temb[i][j] + e1b[c]   (BN already folded), c < c1.
 * All fp32.
 */
int pcd_time_embed(const float* t, int n_t, const float* freqs, int time_dim, int dim,
                   const float* w0, const float* b0, const float* w2, const float* b2,
                   float* temb,
                   const float* e1w_t, const float* e1b, int c1, float* tbias, void* stream);

/* small fp32 linear: y[r][c] = sum_k x[r][k] w[c][k] + b[c]  (emb* layers networks.py:613-618) */
int pcd_linear_f32(const float* x, int rows, int k, const float* w, const float* b, int c,
                   float* y, void* stream);

/* enc1.conv1 xyz half (K=3) + per-shape time bias + ReLU -> fp16 [M][c1]
 * x fp32 [M][3]; w_xyz fp32 [c1][3]; tbias fp32 [n_t][c1] with row index
 * (m / rows_per_shape) * tbias_shape_stride (stride 0 = same t for all shapes; rows are c1 floats, so a
 * stride > 1 walks a wider table whose rows are a multiple of c1 apart). */
int pcd_enc1_xyz(const float* x, int64_t m, int rows_per_shape, const float* w_xyz, int c1,
                 const float* tbias, int tbias_shape_stride, void* out, void* stream);

/* ---------------------------------------------- elementwise diffusion ops (K4)
 * All fp32, bit-exact with the reference's torch-CPU expression order.
 * rates are per shape: r[b * stride], stride 0 or 1. `per_shape` = elements per shape.
 */
/* diffusion.py:151  x_t = s*x0 + n*noise */
int pcd_add_noise(const float* x0, const float* noise, const float* n, const float* s, int stride,
                  int64_t total, int64_t per_shape, float* x_t, void* stream);
/* diffusion.py:167  x0 = (x_t - n*eps)/s */
int pcd_remove_noise(const float* x_t, const float* eps, const float* n, const float* s, int stride,
                     int64_t total, int64_t per_shape, float* x0, void* stream);
/* diffusion.py:283-287 (DDIM):  x0 = (x-n*eps)/s ; x_next = s2*x0 + n2*eps.  x_next may be NULL. */
int pcd_ddim_update(const float* x, const float* eps, const float* n, const float* s,
                    const float* n2, const float* s2, int stride,
                    int64_t total, int64_t per_shape, float* x0, float* x_next, void* stream);
/* diffusion.py:246-255 (DDPM):  x0 as above ; x_next = s2*x0 + coef*n*z */
int pcd_ddpm_update(const float* x, const float* eps, const float* z, const float* n, const float* s,
                    const float* coef, const float* s2, int stride,
                    int64_t total, int64_t per_shape, float* x0, float* x_next, void* stream);
/* pcd_randn_step + pcd_ddpm_update in ONE launch: the step's normal draw z is generated in place (same Philox counters:
 * base_offset + per_step_stride * counter[1] + element / 4, same Box-Muller arithmetic) and never stored; bitwise the two launches. */
int pcd_ddpm_update_philox(const float* x, const float* eps, const float* n, const float* s, const float* coef, const float* s2,
                           int stride, int64_t total, int64_t per_shape, float* x0, float* x_next, uint64_t seed,
                           uint64_t base_offset, uint64_t per_step_stride, const int* counter, void* stream);
/* standard normal fill (Philox4x32-10 + Box-Muller), for perf runs (diffusion.py:239,254,275) */
int pcd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* HIP-graph support: select the per-step constants ON THE DEVICE so one captured step can be
 * replayed for every timestep.  k = counter[0] (clamped to n_steps-1); tb_cur[0..tb_elems) =
 * tb_table[k][:]; rates_cur[t*width + j] = rate_tables[t][k][j] for the 4 tables t (n, s, a, b of
 * the sampler); counter[1] = k; counter[0] = k+1.  counter: device int32[2]. */
int pcd_step_select(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_cur,
                    const float* rate_tables, int width, float* rates_cur, void* stream);
/* pcd_randn whose Philox offset is base_offset + per_step_stride * counter[1] (read on the device) */
int pcd_randn_step(float* out, int64_t n, uint64_t seed, uint64_t base_offset, uint64_t per_step_stride,
                   const int* counter, void* stream);
/* pcd_step_select over `cols` rate tables instead of four (rate_tables [cols][n_steps][width], rates_cur [cols][width]);
 * pcd_step_select is this with cols = 4. */
int pcd_step_select_cols(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_cur,
                         const float* rate_tables, int cols, int width, float* rates_cur, void* stream);

/* ------------------------------------------------ class conditioning with classifier-free guidance (an addition to the
 * reference's surface).  pcd_step_select_cols for a class-conditional run: with the class-bias table class_bias
 * [class_rows][tb_elems] and the device int32 labels[batch] it writes tb_rows [batch + 1][tb_elems]: row b = tb_table[k] +
 * class_bias[labels[b]], row `batch` = tb_table[k] + class_bias[null_row], one fp32 add per element.  The conditional forward
 * reads row 0 with shape stride 1, the unconditional forward row `batch` with stride 0.  A label outside [0, class_rows) is read
 * as null_row.  Rates and counter as pcd_step_select_cols, so one captured step serves every k. */
int pcd_step_select_labels(int* counter, int n_steps, const float* tb_table, int tb_elems, float* tb_rows,
                           const float* class_bias, int class_rows, const int* labels, int batch, int null_row,
                           const float* rate_tables, int cols, int width, float* rates_cur, void* stream);
/* the guidance combine, in place on the conditional prediction: eps[i] = eps_u[i] + w[(i / per_shape) * w_stride] * (eps[i] -
 * eps_u[i]); w_stride 0 (one scale) or 1 (one per shape).  fp32, no FMA contraction: bitwise the expression as written.  16-byte
 * accesses when both pointers are 16-byte aligned (the n % 4 tail element by element), else one element per lane. */
int pcd_cfg_combine(float* eps, const float* eps_u, const float* w, int w_stride, int64_t n, int64_t per_shape, void* stream);

/* ------------------------------------------------ shape completion (an addition to the reference's surface)
 * `PointCloudDiffusion.complete`: shape b knows the first counts[b] rows (of row_elems floats) of p, which has the layout
 * of x; the other rows are generated.  counts: device int32, one per shape.  A row of the step table carries seven
 * per-shape scalars, rates [7][width] read at [c * width + b * stride]: n, s, coef, s_prev (the four of pcd_ddpm_update),
 * n_prev, and the RePaint forward jump ja, jb (ja = 0: the row has no jump).  fp32, no FMA contraction: bitwise
 * tests/completion_statement.py. */
/* start state, in place on the start draw x: known rows become s*p + n*x */
int pcd_complete_start(float* x, const float* p, const int* counts, const float* n, const float* s, int stride,
                       int64_t total, int64_t per_shape, int row_elems, void* stream);
/* one row: x0 = (x - n*eps)/s; x_next = s_prev*x0 + coef*n*z on unknown rows (bitwise pcd_ddpm_update), s_prev*p + n_prev*z
 * on known rows; then, if z2 is given and the row's ja != 0, x_next = ja*x_next + jb*z2.  x_next NULL (the last row):
 * only x0 is written, with its known rows replaced by p.  x_next may be x. */
int pcd_complete_update(const float* x, const float* eps, const float* z, const float* z2, const float* p,
                        const int* counts, const float* rates, int width, int stride, int64_t total,
                        int64_t per_shape, int row_elems, float* x0, float* x_next, void* stream);
/* the same row with z drawn in place from Philox counter base_offset + per_step_stride * counter[1] + element / 4 and, when
 * `jumps` and the row's ja != 0, z2 from that counter + z2_offset (pcd_randn_step's arithmetic; neither is stored).
 * jumps = 0 reads no ja / jb and consumes pcd_ddpm_update_philox's counters. */
int pcd_complete_update_philox(const float* x, const float* eps, const float* p, const int* counts,
                               const float* rates, int width, int stride, int64_t total, int64_t per_shape,
                               int row_elems, int jumps, float* x0, float* x_next, uint64_t seed,
                               uint64_t base_offset, uint64_t per_step_stride, uint64_t z2_offset,
                               const int* counter, void* stream);

/* ------------------------------------------------ second-order multistep sampler (an addition to the reference's surface)
 * One step of `sample_dpm` (DPM-Solver++ 2M, data-prediction form).  rates [6][width] read at [c * width + b * stride]:
 * n, s, n_next, s_next, c, q with q = s / n and c = h_k / (2 h_{k-1}) (0 on the first step and for order 1).
 *   x0 = (x - n*eps)/s;  w = c*(x0 - hist);  D = x0 + w;  eD = eps - q*w;  x_next = s_next*D + n_next*eD;  hist = x0
 * hist holds the previous step's x0 and receives this step's, in place.  c = 0: hist is not read (it may be unwritten) and
 * x0, x_next are bitwise pcd_ddim_update's.  x_next NULL: only hist = x0 is written.  x_next may be x.  fp32, no FMA
 * contraction: bitwise tests/dpm_statement.py. */
int pcd_dpm_update(const float* x, const float* eps, const float* rates, int width, int stride, int64_t total,
                   int64_t per_shape, float* hist, float* x_next, void* stream);

/* output head: eps[m][j] = sum_k h[m][k]*w[j][k] + b[j], j<3  (networks.py:770 `output.3`),
 * h fp16 [M][k], w fp32 [3][k]; eps fp32 [M][3]. */
int pcd_head3(const void* h, int64_t m, int k, const float* w, const float* b, float* eps, void* stream);

/* ------------------------------------------------ whole point denoiser (a7)
 * UNetPointNetLarge.forward (networks.py:779-818) as one enqueue of ~30 kernels.
 * The descriptor holds device pointers to host-folded weights (BN folded, refine_k folded
 * into dec_k.conv1, time/global halves hoisted: SURVEY.md A.3).
 */
#define PCD_UNET_NLIN 26
typedef struct {
    const void* w; const float* b; int k; int c;
} pcd_linear_desc_t;

typedef struct {
    int time_dim, dim;
    const float* freqs;                       /* [time_dim/2] */
    const float *tw0, *tb0, *tw2, *tb2;       /* time_mlp fp32 */
    const float* e1w_xyz;                     /* [64][3]  */
    const float* e1w_t;                       /* [64][dim] */
    const float* e1b;                         /* [64] */
    pcd_linear_desc_t lin[PCD_UNET_NLIN];     /* execution order, see csrc/unet.hip */
    const void* wg; int wg_k, wg_c;           /* dec4.conv1 global-feature half fp16 [1024][4096] */
    const float* head_w; const float* head_b; /* output.3 fp32 [3][64], [3] */
    unsigned hilo_mask;                       /* bit i: lin[i].w is [c][2 k] = the fp16 weights | the fp16 of their rounding residuals
                                                 (hi / lo weights, ~22 bits): allowed for the narrow layers PCD_UNET_HILO_ALLOWED */
} pcd_unet_desc_t;
/* layers that may carry hi / lo weights: enc1.conv2, enc1.conv3 (0, 1), enc2.conv3 (4), dec1.conv1 .. output.0 (22 .. 25) */
#define PCD_UNET_HILO_ALLOWED 0x3C00013u

/* Chains of the narrow pointwise layers of UNetPointNetLarge in one launch each (csrc/chain.hip): a wave carries 32
 * points through the chain with the intermediates in LDS, the chain's weights (fp16 [C][K], BatchNorm folded) resident
 * in LDS.  Every layer = Conv1d(k=1) + BN + ReLU with fp32 accumulation and one fp16 rounding, like pcd_gemm_f16.
 *   enc1:  x fp32 [m][3] -> conv1 (K = 3, + per-shape time bias, as pcd_enc1_xyz) -> conv2 64->64 -> conv3 64->128 -> x1
 *   128:   in fp16 [m][128] -> 128->128 -> 128->128 -> out fp16 [m][128]                 (enc2.conv1, enc2.conv2)
 *   tail:  in fp16 [m][128] -> 128->128 -> 128->64 -> 64->64 -> 64->3 fp32 (no ReLU)     (dec1.conv2, conv3, output.0, output.3) */
int pcd_pw_chain_enc1(const float* x, int64_t m, int rows_per_shape, const float* w_xyz, const float* tbias,
                      int tbias_shape_stride, const void* w_conv2, const float* b_conv2, const void* w_conv3,
                      const float* b_conv3, void* x1, void* stream);
int pcd_pw_chain_128(const void* in, int64_t m, const void* w_a, const float* b_a, const void* w_b, const float* b_b,
                     void* out, void* stream);
int pcd_pw_chain_tail(const void* in, int64_t m, const void* w_a, const float* b_a, const void* w_b, const float* b_b,
                      const void* w_c, const float* b_c, const float* head_w, const float* head_b, float* eps, void* stream);
/* enc1 and tail chains with hi / lo weights (every w_* is [C][2 K] = hi | lo; see pcd_gemm_f16_hilo): the same arithmetic with the K
 * loop run against hi, then against lo.  These narrow layers are the direct route from the coordinates to the predicted noise; the
 * fp16 rounding of their weights is what the fp16 path's 1000-step DDPM trajectory deviates by. */
int pcd_pw_chain_enc1_hilo(const float* x, int64_t m, int rows_per_shape, const float* w_xyz, const float* tbias,
                           int tbias_shape_stride, const void* w_conv2, const float* b_conv2, const void* w_conv3,
                           const float* b_conv3, void* x1, void* stream);
int pcd_pw_chain_tail_hilo(const void* in, int64_t m, const void* w_a, const float* b_a, const void* w_b, const float* b_b,
                           const void* w_c, const float* b_c, const float* head_w, const float* head_b, float* eps, void* stream);
/* One pointwise layer out[m][c] = act(in[m][k] . W^T + bias) with the weights resident in LDS: the 1x1x1 shortcut
 * convolutions of ResidualBlock3D (reference networks.py:485-490) on NDHWC rows.  in fp16 [m][k]; w fp16 [c][ldw] (k used);
 * bias fp32 [c]; relu 0/1; out fp16 [m][c].  Shapes: (k, c) = (32, 64), (64, 128), (128, 256) -- pcd_conv1x1_supported(). */
int pcd_conv1x1_supported(int k, int c);
int pcd_conv1x1_f16(const void* in, int64_t m, int k, const void* w, int64_t ldw, const float* bias, int relu, int c,
                    void* out, void* stream);
/* testing / tuning hook for pcd_unet_forward, a mask: bit 0 = the narrow chained kernels above, bit 1 = the 256-channel chains and the row-panel chains
 * below, bit 2 = the row-panel chains OFF (so 3, the default, is everything on; 7 = everything but the row-panel chains; 1 and 0 = per-layer GEMMs there),
 * bit 3 = D43 OFF: dec4.conv3 and dec3.conv1 as per-layer launches in front of D3T (11 = everything but D43) */
int pcd_unet_config(int use_chains);
/* Row-panel chains (csrc/panelchain.hip): consecutive 512-channel-input store layers as one launch with the activations of a 128-row panel resident in
 * LDS.  chain 0 (E4): enc4.conv1-3, x [M][512] -> out [M][ld >= 1024]; chain 1 (D3T): dec3.conv2-3, x [M][512] -> out [M][ld >= 256].  frag[l] =
 * pcd_gemm_pack_wfrag's copy of layer l's [C][512] weights, bias[l] fp32 [C] (3 layers / 2 layers); every layer ends in ReLU.  hilo: bit l set = layer l
 * has hi | lo weights.  cap = the most workgroups (1 .. 256).  Bitwise the per-layer pcd_gemm_f16 launches.  Refuses (PCD_ERR_ARG, nothing launched)
 * M % 128 != 0, a null fragment copy, hilo != 0, out == x. */
int pcd_panel_chain(int chain, const void* x, int64_t m, const void* const* frag, const float* const* bias, int hilo, void* out, int64_t ld, int cap,
                    void* stream);
/* The same kernel over dec4.conv3, dec3.conv1-3 (D43: lin 15, 16, 17, 18): x [M][1024] and x3 [M][512] -> out [M][ld >= 256].  The two K = 1024 layers
 * read their first K half from the resident panel while the second half (columns 512 .. 1023 of x; x3) rolls into the K-tile images already read.
 * frag[0], frag[1] = pcd_gemm_pack_wfrag's copies of [512][1024] weights (lin 16's K is [lin 15's output | x3]), frag[2], frag[3] of [512][512] and
 * [256][512]; bias[l] fp32 [C]; every layer ends in ReLU.  Bitwise the per-layer pcd_gemm_f16 launches.  Refuses (PCD_ERR_ARG, nothing launched)
 * M % 128 != 0, a null fragment copy, hilo != 0, out == x or out == x3. */
int pcd_panel_chain_dec(const void* x, const void* x3, int64_t m, const void* const* frag, const float* const* bias, int hilo, void* out, int64_t ld,
                        int cap, void* stream);
/* The 256-channel chains of the same network as one launch each (csrc/widechain.hip): chain 0 = enc3.conv1-3 (x2 [M][256] -> x3 [M][512]),
 * chain 1 = dec2.conv1-3 ([in1 [M][256] | in2 [M][256]] -> [M][128]).  A wave carries 32 points through the chain with the activations
 * in registers (the layer-to-layer hand-over is a v_permlane32_swap per register); only the weights stream, as 32-KB stage images that
 * pcd_pw_wide_pack builds once from the three layers' [C][K] fp16 weights and fp32 biases (BatchNorm folded, as for pcd_gemm_f16) into a
 * caller-owned buffer of pcd_pw_wide_packed_bytes(chain) bytes.  M must be a multiple of 256.  pcd_unet_config bit 1 switches
 * pcd_unet_forward between these chains and one GEMM launch per layer (bit 0: the narrow chains above). */
size_t pcd_pw_wide_packed_bytes(int chain);
int pcd_pw_wide_pack(int chain, const void* const* w, const float* const* b, void* packed, void* stream);
int pcd_pw_wide_chain(int chain, const void* in1, const void* in2, int64_t m, const void* packed, void* out, void* stream);
/* A/B hook (TEST / BENCHMARK ONLY, process-global): which waves request the weight images of the wide-chain launches (1, default: one wave per SIMD,
 * alternating groups per image; 0: every wave; 2: the split form in the LN + Linear launches too).  Same bits either way. */
int pcd_pw_wide_config(int split);
/* The narrow ends of the same network on the same engine, with a shape per segment (K, C in {128, 256}; a stage image is 256 channels x 64 k or
 * 128 channels x 128 k), one launch each:
 *   chain 0 (E23): in1 = x1 [M][128] -> enc2.conv1 -> conv2 -> conv3 -> enc3.conv1 -> conv2 -> conv3; out = x3 [M][512], out2 = x2 [M][256] (stored for
 *                  the decoder's skip, never read back); w[0..5] / b[0..5] = the six layers; in2, in3 unused;
 *   chain 1 (D21): [in1 [M][256] | in2 = x2 [M][256]] -> dec2.conv1 -> conv2 -> conv3 -> dec1.conv1 on [that (128, in registers) | in3 = x1 [M][128]];
 *                  out [M][128]; w[0..3] / b[0..3]; out2 unused.
 * hilo != 0: the chain's narrow layer (enc2.conv3 / dec1.conv1) has [c][2 k] hi | lo weights: all hi K passes, then all lo passes onto the same
 * accumulators, as in pcd_gemm_f16_hilo.  packed: pcd_pw_wide_ends_packed_bytes(chain, hilo) bytes, built once by pcd_pw_wide_ends_pack.  M % 256 == 0.
 * pcd_pw_wide_config chooses the request form of the weight ring here too. */
size_t pcd_pw_wide_ends_packed_bytes(int chain, int hilo);
int pcd_pw_wide_ends_pack(int chain, int hilo, const void* const* w, const float* const* b, void* packed, void* stream);
int pcd_pw_wide_ends(int chain, int hilo, const void* in1, const void* in2, const void* in3, int64_t m, const void* packed, void* out, void* out2,
                     void* stream);
/* LayerNorm(256) + Linear(256, 256 passes) [+ ReLU] as one launch of the wide-chain kernel (csrc/widechain.hip): the B fragments are normalised as they
 * are loaded (two-pass fp32 statistics, eps 1e-5, fp16 result as pcd_layernorm_f16's), so the LayerNorm launch and its tensor disappear: attention in_proj
 * (passes 3, relu 0) and ff.0 (passes 4, relu 1) of the C = 256 SetAttentionBlocks (networks.py:61-66, 81-82).  w fp16 [256 passes][256], b fp32;
 * packed: pcd_pw_wide_ln_linear_packed_bytes(passes) bytes of device memory; rows % 256 == 0; out fp16 [rows][256 passes], out != x. */
size_t pcd_pw_wide_ln_linear_packed_bytes(int passes);
int pcd_pw_wide_ln_linear_pack(const void* w, const float* b, int passes, const float* ln_g, const float* ln_b, void* packed, void* stream);
int pcd_pw_wide_ln_linear_supported(int dim, int64_t rows);
int pcd_pw_wide_ln_linear(const void* packed, int passes, int relu, const void* x, int64_t rows, void* out, void* stream);

typedef struct pcd_unet pcd_unet_t;
int pcd_unet_create(const pcd_unet_desc_t* desc, pcd_unet_t** out);
void pcd_unet_destroy(pcd_unet_t* h);
size_t pcd_unet_workspace_bytes(int batch, int n_points);
/* eps = model(x, t):  x fp32 [B][N][3]; tbias fp32 [n_t][64] from pcd_time_embed with
 * tbias_shape_stride 0 (one t for the batch) or 1 (one per shape); eps fp32 [B][N][3]. */
int pcd_unet_forward(pcd_unet_t* h, const float* x, int batch, int n_points,
                     const float* tbias, int tbias_shape_stride,
                     float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* HIP-event timing of the dominant kernel (global_feat.3 GEMM + max) on the launch stream:
 * enable, run forwards, then read the summed duration and launch count (bench.py roofline). */
int pcd_unet_profile(pcd_unet_t* h, int enable);
int pcd_unet_profile_read(pcd_unet_t* h, double* total_ms, int* launches);
/* optional taps for parity tests: copies of x1..x4 (fp16), pooled / gbias (fp32) out of the last forward's workspace */
int pcd_unet_tap(pcd_unet_t* h, const char* name, int batch, int n_points,
                 const void* workspace, void* dst, size_t dst_bytes, void* stream);
/* The decoder blocks' outputs (reference networks.py:811-814: dec4 [M][512], dec3 [M][256], dec2 [M][128], dec1 [M][64], fp16)
 * live in ping-pong buffers / inside the chained tail; while capture buffers are set, every forward copies them out
 * (dec1: the tail runs as per-layer launches, bit-identical).  Null pointers switch the capture off. */
int pcd_unet_capture(pcd_unet_t* h, void* d4, void* d3, void* d2, void* d1);

/* ------------------------------------------------ fp32 parity mode of the point denoiser (csrc/unet_f32.hip)
 * SURVEY 8(c) "HIP fp32 parity mode": the network of pcd_unet_forward with fp32 weights, fp32 activations and fp32
 * products (v_mfma_f32_32x32x2_f32); same descriptor layout and lin[] order, but EVERY weight pointer (lin[i].w, wg) is
 * fp32 [C][K].  Held to eps rel-L2 <= 1e-4 per forward against the reference's fp32 arithmetic (networks.py:779-818).
 * pcd_gemm_f32: out[m][c] = act([A1 | A2][m][k1 + k2] . W[c][k]^T + bias[c] (or shape_bias[row / rows_per_shape][c]));
 * k1, k2 multiples of 16.  pcd_gemm_f32_colmax: pooled[row / rows_per_shape][c] = max(pooled, relu(A . W^T + bias)), the
 * `torch.max(x, 2)` of networks.py:807 fused (pooled zero-initialised by the caller).
 * Taps of the last forward (all fp32): x1..x4, pooled, gbias, d4..d1. */
int pcd_gemm_f32(const float* a1, int64_t lda1, int k1, const float* a2, int64_t lda2, int k2, const float* w, int64_t ldw,
                 const float* bias, const float* shape_bias, int rows_per_shape, int relu, int m, int c, float* out,
                 int64_t ldo, void* stream);
int pcd_gemm_f32_colmax(const float* a, int64_t lda, int k, const float* w, int64_t ldw, const float* bias, int m, int c,
                        float* pooled, int rows_per_shape, void* stream);
typedef struct pcd_unet_f32 pcd_unet_f32_t;
int pcd_unet_f32_create(const pcd_unet_desc_t* desc, pcd_unet_f32_t** out);
void pcd_unet_f32_destroy(pcd_unet_f32_t* h);
size_t pcd_unet_f32_workspace_bytes(int batch, int n_points);
int pcd_unet_f32_forward(pcd_unet_f32_t* h, const float* x, int batch, int n_points, const float* tbias,
                         int tbias_shape_stride, float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* diagnostic: bit i of `mask` makes lin[i]'s output (bit 26: enc1.conv1's) round to fp16 and back before it is stored, everything else
 * staying fp32 -- locates where ACTIVATION rounding of the fp16 product path matters (tools/attribute_fp16_layers.py); 0 = off */
int pcd_unet_f32_round_activations(pcd_unet_f32_t* h, unsigned mask);
int pcd_unet_f32_tap(pcd_unet_f32_t* h, const char* name, int batch, int n_points, const void* workspace, void* dst,
                     size_t dst_bytes, void* stream);

/* ------------------------------------------------ latent denoiser (a11, K8)
 * GroupNorm(groups, C, eps 1e-5, biased var) + affine + ReLU on rows of x fp32 [rows][c] -> fp16
 * (the Linear+GroupNorm(8)+ReLU stages of networks.py:984-1036; 2-D input = per-sample groups). */
int pcd_groupnorm_relu_f16(const float* x, int rows, int c, int groups, const float* gamma,
                           const float* beta, void* out, void* stream);
/* Weight-streaming GEMM for M <= 256 rows (the latent vectors): split-K partial sums
 * slabs[s][m][c] = sum over the s-th K slice of [A1|A2][m][k] * W[c][k]; pcd_skinny_slabs gives S.
 * pcd_skinny_finish adds the slabs in a fixed order (+bias, + optional per-row bias) and applies
 * mode 0: GroupNorm(groups)+affine+ReLU -> fp16, 1: ReLU -> fp16, 2: identity -> fp32. */
int pcd_skinny_slabs(int k, int c);
int pcd_skinny_gemm_f16(const void* a1, int k1, const void* a2, int k2, const void* w, int64_t ldw,
                        int m, int c, float* slabs, void* stream);
/* the same with one fp32 activation matrix a [m][k], rounded to fp16 (saturating, as pcd_f32_to_f16) as it is loaded: the same slabs bit for bit
 * as pcd_f32_to_f16 followed by pcd_skinny_gemm_f16 (the pooled maxima of pcd_unet_forward) */
int pcd_skinny_gemm_f32in(const float* a, int k, const void* w, int64_t ldw, int m, int c, float* slabs, void* stream);
int pcd_skinny_finish(const float* slabs, int nslabs, int m, int c, const float* bias, const float* row_bias,
                      int mode, int groups, const float* gamma, const float* beta,
                      void* out16, float* out32, void* stream);
/* testing / tuning hook: use_lds_dma = 0 makes the skinny kernels load their MFMA fragments straight from global memory
 * (the first form) instead of staging full 128-byte lines through LDS by LDS-DMA; 1 restores the default.  Same bits. */
int pcd_skinny_config(int use_lds_dma);
/* The same layer in ONE launch for small weights (k * c <= 768 * 256): a workgroup owns whole GroupNorm groups
 * over the full K, so Linear + bias + GroupNorm + ReLU need no second kernel (enc1-3, dec1-2 and the output head of
 * SimpleLatentUNetPointNet, networks.py:984-1049).  pcd_skinny_fused_supported() tells (1/0) whether a shape
 * qualifies (mode 0: group size 16/32/64/128). */
int pcd_skinny_fused_supported(int k, int c, int mode, int groups);
int pcd_skinny_fused(const void* a1, int k1, const void* a2, int k2, const void* w, int64_t ldw, int m, int c,
                     const float* bias, const float* row_bias, int mode, int groups, const float* gamma,
                     const float* beta, void* out16, float* out32, void* stream);
/* ... with the activations given in fp32 [m][k] and rounded to fp16 on load (enc1 reads the latent state z directly;
 * saves the separate conversion launch). */
int pcd_skinny_fused_f32in(const float* a, int k, const void* w, int64_t ldw, int m, int c, const float* bias,
                           const float* row_bias, int mode, int groups, const float* gamma, const float* beta,
                           void* out16, float* out32, void* stream);
/* SimpleLatentUNetPointNet.forward (networks.py:1051-1086), latent_dim=256, dim=512, time_dim=256.
 * lin[] order documented in csrc/latent.hip; refine_k folded into dec_k, enc1's time half hoisted
 * into tbias [n_t][128] (pcd_time_embed with c1=128). */
#define PCD_LATENT_NLIN 12
typedef struct {
    pcd_linear_desc_t lin[PCD_LATENT_NLIN];
    const float* gn_gamma[PCD_LATENT_NLIN];   /* entries 0..9 (GroupNorm layers), rest NULL */
    const float* gn_beta[PCD_LATENT_NLIN];
} pcd_latent_desc_t;
typedef struct pcd_latent pcd_latent_t;
int pcd_latent_create(const pcd_latent_desc_t* desc, pcd_latent_t** out);
void pcd_latent_destroy(pcd_latent_t* h);
size_t pcd_latent_workspace_bytes(int batch);
/* eps = model(z, t): z fp32 [B][256] -> eps fp32 [B][256]; tbias stride 0 (one t) or 1 (per sample) */
int pcd_latent_forward(pcd_latent_t* h, const float* z, int batch, const float* tbias,
                       int tbias_shape_stride, float* eps, void* workspace, size_t workspace_bytes,
                       void* stream);

/* fp32 parity mode of the latent denoiser (csrc/latent_f32.hip): pcd_latent_forward's network with fp32 weights (EVERY
 * lin[i].w of the descriptor is fp32 [C][K] here), fp32 activations and products, one launch per layer and GroupNorm;
 * held to eps rel-L2 <= 1e-4 against the reference's fp32 arithmetic (networks.py:1051-1086). */
typedef struct pcd_latent_f32 pcd_latent_f32_t;
int pcd_latent_f32_create(const pcd_latent_desc_t* desc, pcd_latent_f32_t** out);
void pcd_latent_f32_destroy(pcd_latent_f32_t* h);
size_t pcd_latent_f32_workspace_bytes(int batch);
int pcd_latent_f32_forward(pcd_latent_f32_t* h, const float* z, int batch, const float* tbias, int tbias_shape_stride,
                           float* eps, void* workspace, size_t workspace_bytes, void* stream);

/* The same network, and whole DDIM timesteps of the latent sampler (the loop body of LatentDiffusion.sample / sample3,
 * diffusion.py:637-645, 691-700), as ONE persistent launch for batch <= 64 (csrc/latent_persist.hip; 33 .. 64 rows run as two interleaved streams of <= 32): 256 workgroups, one
 * per CU, keep all 38 MB of fp16 weights in LDS for the whole call and exchange activations through self-validating
 * buffers (no flags or atomics between layers).  pcd_latent_persist_supported(batch) tells (1/0) whether the current
 * device can run it (exactly 256 CUs with 160 KB LDS, batch <= 64); callers fall back to pcd_latent_forward otherwise.
 * The handle keeps the descriptor's pointers.  Workspace: pcd_latent_persist_workspace_bytes(h), 256-byte aligned, owned
 * by the caller, private to one in-flight call.
 *  - pcd_latent_persist_forward: eps = model(z, t) with tbias = the hoisted time row [128] (one t for the batch).
 *  - pcd_latent_persist_ddim: `nsteps` consecutive DDIM steps starting at table row counter[0] (pcd_step_select
 *    semantics: rows clamp at n_steps_table - 1; on return counter[0] += nsteps, counter[1] = last row used): z is
 *    updated in place, x0 (may be NULL) receives the last step's x0.  rate_tables is (4, n_steps_table, rate_width)
 *    fp32 = (n, s, n_next, s_next) like pcd_ddim_update's operands, rate_width 1 or batch.  The update is bitwise
 *    pcd_ddim_update's.
 *  - every in-kernel wait is bounded (0.2 s); pcd_latent_persist_status waits for the launch stream and copies the status word to the
 *    host: 0 = ok, otherwise (wait kind << 16 | workgroup) of the first wait that gave up (outputs
 *    are then undefined).
 *  - pcd_latent_persist_config: tuning hooks: poll back-off (s_sleep count between polls); predict_waits = 1 (default): a wait
 *    sleeps through 7/8 of the time the same wait took in the previous step before it starts probing. */
typedef struct pcd_latent_persist pcd_latent_persist_t;
int pcd_latent_persist_supported(int batch);
int pcd_latent_persist_create(const pcd_latent_desc_t* desc, pcd_latent_persist_t** out);
void pcd_latent_persist_destroy(pcd_latent_persist_t* h);
size_t pcd_latent_persist_workspace_bytes(const pcd_latent_persist_t* h);
int pcd_latent_persist_config(pcd_latent_persist_t* h, int poll_sleep, int predict_waits);
/* diagnostic: instrumented kernel for the next launches; buf [256][steps][8 units][8] u32 of 100 MHz stamps, NULL = off */
int pcd_latent_persist_trace(pcd_latent_persist_t* h, unsigned* buf, int steps);
int pcd_latent_persist_forward(pcd_latent_persist_t* h, const float* z, int batch, const float* tbias, float* eps,
                               void* workspace, size_t workspace_bytes, void* stream);
int pcd_latent_persist_ddim(pcd_latent_persist_t* h, float* z, float* x0, int batch, const float* tb_table, int tb_elems,
                            const float* rate_tables, int rate_width, int n_steps_table, int* counter, int nsteps,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Class-conditional forms of the two launches above (classifier-free guidance; the arithmetic is tests/latent_cfg_statement.py).
 * A row's enc1 bias is the step's time row + class_bias[c], class_bias (class_rows, 128) fp32 = the class table through enc1's
 * time columns, c = labels[shape] (a value outside [0, class_rows) reads null_row, as pcd_step_select_labels does).
 *  - w == NULL: labelled only.  Rows map as in the unlabelled launches (batch <= 64).
 *  - w != NULL (batch <= 32): a 32-row tile carries up to 16 shapes, local row r < 16 the shape with its label and row r + 16 the
 *    same state with the null class; output.2's epilogue forms eps = eps_u + w (eps_c - eps_u) (pcd_cfg_combine's operation order;
 *    w[shape * w_stride], w_stride 0 or 1) before the update, so both rows publish the same next state.  17 .. 32 shapes run as
 *    the two interleaved streams.
 * No new buffers or workspace bytes.  With a trace buffer set (pcd_latent_persist_trace) both return PCD_ERR_ARG.
 *  - pcd_latent_persist_forward_guided: eps (batch, 256) = the guided eps, or the conditional eps when w == NULL. */
int pcd_latent_persist_ddim_guided(pcd_latent_persist_t* h, float* z, float* x0, int batch, const float* tb_table, int tb_elems,
                                   const float* class_bias, int class_rows, int null_row, const int* labels, const float* w,
                                   int w_stride, const float* rate_tables, int rate_width, int n_steps_table, int* counter,
                                   int nsteps, void* workspace, size_t workspace_bytes, void* stream);
int pcd_latent_persist_forward_guided(pcd_latent_persist_t* h, const float* z, int batch, const float* tbias_row,
                                      const float* class_bias, int class_rows, int null_row, const int* labels, const float* w,
                                      int w_stride, float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* waits for `stream` (the stream the launch was enqueued on; nothing else is synchronised), then reads the status word of the last launch:
 * 0 = every wait was met; else (wait kind << 16) | workgroup.
 * A non-zero status means the launch was ABANDONED (its outputs are undefined): the caller re-runs from its saved input on
 * the per-layer path (shapegen_amd.diffusion.LatentDiffusion._run does). */
int pcd_latent_persist_status(const void* workspace, unsigned* status_host, void* stream);
/* fault injection for the recovery tests: in the following launches workgroup `workgroup` (role index 0..255) leaves at the
 * start of step `step`, as a workgroup that never became resident would; workgroup < 0 switches it off. */
int pcd_latent_persist_inject_fault(pcd_latent_persist_t* h, int workgroup, int step);
/* host-only self check of the kernel's static work assignment (no device needed): bytes of one buffer set, or -1 */
int pcd_latent_persist_plan_check(void);
/* host-only: phase id (2 * layer + finish, -1 = none) of every workgroup's units, [256][8] ints */
int pcd_latent_persist_plan_dump(int* phases_host);

/* ------------------------------------------------------ 3-D convolution (a12, K9)
 * Implicit-GEMM Conv3d on NDHWC fp16 activations (replaces nn.Conv3d / nn.ConvTranspose3d +
 * BatchNorm3d(eval) + ReLU / residual add of networks.py:2225-2264, 471-504; BN folded on the host).
 * Rows m enumerate (b, oz, oy, ox) over rows_d x rows_h x rows_w; tap t reads input voxel
 * (oz*stride+dz_t, oy*stride+dy_t, ox*stride+dx_t) (zero outside the grid) and multiplies
 * w[cout][t*cin .. t*cin+cin); K = ntaps*cin zero-padded to kpad (multiple of 64).
 * Output voxel = (oz*out_scale+out_off_z, ...) of an out_d x out_h x out_w grid, so one
 * output-parity class of ConvTranspose3d(k4,s2,p1) is a 2x2x2-tap call with out_scale 2.
 * out = relu?( conv + bias (+ resid) ).  taps: device int32 [ntaps], bytes (dz, dy, dx, 0) signed.
 */
typedef struct {
    const void* in; int batch, in_d, in_h, in_w, cin;      /* fp16 [B][D][H][W][cin], cin power of two >= 8 */
    int rows_d, rows_h, rows_w, stride;
    const int* taps; int ntaps, kpad;
    const void* w; const float* bias;                      /* fp16 [cout][kpad], fp32 [cout] */
    const void* resid; int relu;                           /* optional fp16 residual indexed like out */
    void* out; int cout;                                   /* fp16 [B][out_d][out_h][out_w][cout], cout % 8 == 0 */
    int out_d, out_h, out_w, out_scale, out_off_z, out_off_y, out_off_x;
    const void* zero_page;                                 /* >= 128 bytes of zeros */
    /* optional SECOND SOURCE (NULL = none): fp16 [B][rows_d][rows_h][rows_w][cin2] on the row grid; K columns
     * [ntaps*cin, ntaps*cin + cin2) of w multiply row m of in2 -- a 1x1x1 convolution of another tensor summed into the same
     * accumulators, which is how ResidualBlock3D's projection shortcut (networks.py:485-490, 500-503) rides in conv2's launch:
     * relu(bn2(conv2 h) + downsample(x)) = relu([gather(h) | x] . [W2 | Wds]^T + b2 + bds), one fp16 rounding, no shortcut
     * tensor.  Needs stride 1, out_scale 1, rows == in dims, resid NULL, ntaps*cin % 64 == 0; the implicit GEMM takes cin2 a
     * power of two >= 64 with kpad == ntaps*cin + cin2, the k3s1 halo kernel cin 64, cout % 64 == 0 with cin2 == 32. */
    const void* in2; int cin2;
} pcd_conv3d_desc_t;
int pcd_conv3d_f16(const pcd_conv3d_desc_t* d, void* stream);
/* n (1..8) problems in ONE launch that share everything except taps, w and out_off_* -- the 2x2x2
 * output-parity classes of ConvTranspose3d(k4, s2, p1) (networks.py:2243,2248,2253) -- and, when the
 * launch would leave the chip mostly idle (few output rows, long K: encoder.9-12, decoder.0), split-K
 * over blockIdx.z with fp32 partial slabs in `workspace`, summed in split order by a finish kernel that
 * applies the same bias/residual/ReLU epilogue.  pcd_conv3d_workspace_bytes() returns the scratch that
 * split needs (0 = the launch is not split); with a NULL/short workspace the launch runs unsplit. */
size_t pcd_conv3d_workspace_bytes(const pcd_conv3d_desc_t* descs, int n);
int pcd_conv3d_f16_multi(const pcd_conv3d_desc_t* descs, int n, void* workspace, size_t workspace_bytes,
                         void* stream);
/* Which of the convolution kernels run.  TEST / BENCHMARK ONLY: process-global, not synchronised with launches in flight.
 * code = the sum of one value per field; 1 is the library's default; PCD_ERR_ARG unless 0 <= code < 262144 and (code & 7) <= 2.
 *
 *   bits    value        effect
 *   0-2     0            pcd_conv3d_k3s1_f16 at C_in = 32, C_out <= 32: 128-row workgroups
 *           1 (default)  256-row workgroups (4 x 8 x 8 voxels, eight waves) where the grid has at least 512 of them
 *           2            256-row workgroups wherever H % 8 == 0 (tests).  Same bits in all three.
 *   3-4     0 (default)  pcd_conv3d_last_sigmoid_packed: per-tap partial products on the matrix pipe (the fp32 weights as fp16 hi + lo + lo2 parts)
 *           + 8          4 x 4 x 8 blocks on the VALU (fp32 weights)
 *           + 16         8 x 8 x 8 blocks on the VALU (fp32 weights)
 *           + 24         8 x 8 x 8 blocks with one MFMA per tap and 16 voxels (from the packed copy).  The forms agree to 1e-6.
 *   5-6     0 (default)  split-K aims at 512 workgroups
 *           + 32 / + 64 / + 96   at 768 / 384 / 1024 (all measured slower on VAE3DLarge)
 *   7-8     + 128, + 256 timing ablations 1, 2 of the per-tap last-layer kernel (OUTPUTS WRONG); + 384 runs the real kernel
 *   9       + 512        pcd_conv3d_first on 4 x 4 x 8 tiles where 8 x 8 x 8 would fit (same bits)
 *   10-13   + 1024 x a   timing ablation a of the 128 x 128 implicit GEMM: 1 / 2 operand staging, 4 fragment reads, 8 MFMAs; the sums 3, 7, 15 of
 *                        them are built too, any other a runs the real kernel (OUTPUTS WRONG)
 *   14      + 16384      per-tap last layer with a wave per output slice instead of a wave per four 8 x 8 slices that reads every input slice once
 *   15-17   + 32768 x a  timing ablation a of conv3d_halo_wreg_kernel<64, 2>: 1 halo not loaded, 2 no halo staging, 4 no taps; 6 is built too, any
 *                        other a runs the real kernel (OUTPUTS WRONG) */
int pcd_conv3d_config(int code);
/* Conv3d(k3, stride 1, pad 1) (+ folded BN, residual, ReLU) with the input halo of a 4x4x8 output block held in
 * LDS and reused by all 27 taps -- the 32^3 layers of VAE3DLarge (encoder.2, decoder.8-11; networks.py:2227,
 * 2256-2259), whose gather traffic bounds the generic kernel.  Same descriptor; the tap table is implied
 * (regular 3x3x3, (kz, ky, kx) order, offsets -1..1) and d->taps is not read.  Supported: cin 32 or 64, spatial
 * dims multiples of (4, 4, 8), out_scale 1; pcd_conv3d_k3s1_supported() tells (1/0), unsupported -> PCD_ERR_ARG. */
int pcd_conv3d_k3s1_supported(const pcd_conv3d_desc_t* d);
int pcd_conv3d_k3s1_f16(const pcd_conv3d_desc_t* d, void* stream);
/* Conv3d(k3, stride 1, pad 1), C_in = 128, 64 or 32, with the weights in registers (csrc/conv3d_halo.hip: conv3d_halo_wreg_kernel): the same function and descriptor as
 * pcd_conv3d_k3s1_f16 (bias, residual, ReLU; d->w / d->kpad / d->taps are not read), the weights given in MFMA-fragment order -- wfrag, made once per
 * layer by pcd_conv3d_pack_wfrag from the [cout][kpad] matrix (pcd_conv3d_wfrag_bytes(cin, cout) bytes).  A workgroup owns 4 x 8 x 8 output voxels with their
 * halo in LDS; weight fragments are coalesced 1-KB global loads straight into MFMA operand registers; no barrier in the tap loop.  Supported: cin 128 (eight
 * waves over a 153.6-KB halo, cout % 128 == 0), 64 or 32 (cout 32 or a multiple of 64), dims multiples of (4, 8, 8), at cin >= 64 a second source of cin2 = 32 or
 * 64 channels (pack with the same cin2) (its weight columns are "tap 27" of wfrag, its rows come straight
 * from global memory); pcd_conv3d_k3s1_wreg_supported() tells.  Same sums in the same k order as
 * pcd_conv3d_k3s1_f16 per accumulator (bitwise the same outputs). */
size_t pcd_conv3d_wfrag_bytes(int cin, int cout);
int pcd_conv3d_pack_wfrag(const void* w, int kpad, int cin, int cout, int cin2, void* wfrag, void* stream);
int pcd_conv3d_k3s1_wreg_supported(const pcd_conv3d_desc_t* d);
int pcd_conv3d_k3s1_wreg_f16(const pcd_conv3d_desc_t* d, const void* wfrag, void* stream);
/* Conv3d(k4, s2, p1) (+ folded BN) (+ ReLU) with LDS-resident input (encoder.3/4, networks.py:2229-2230; csrc/conv3d_halo.hip: conv3d_k4s2_halo_kernel):
 * in fp16 [B][d][h][w][cin], w fp16 [cout][kpad] in the tap-major layout of pcd_conv3d_f16 (k = ((kz * 4 + ky) * 4 + kx) * cin + c), out fp16
 * [B][d/2][h/2][w/2][cout].  The kernel walks the eight input-parity classes (each a 2 x 2 x 2 stride-1 convolution of one sub-sampled grid) of a
 * 4 x 4 x 8 output block with that class's sub-grid halo in LDS.  Supported: cin 64, cout 64, d, h, w multiples of (8, 8, 16) and <= 64;
 * pcd_conv3d_k4s2_halo_supported() tells (1 / 0), unsupported -> PCD_ERR_ARG.  Same sums as pcd_conv3d_f16 in another order (exact on integers). */
int pcd_conv3d_k4s2_halo_supported(int batch, int d, int h, int w, int cin, int cout, int kpad);
int pcd_conv3d_k4s2_halo_f16(const void* in, int batch, int d, int h, int w, int cin, const void* wgt, int kpad, const float* bias, int relu,
                             int cout, void* out, void* stream);
/* ConvTranspose3d(k4, s2, p1) + ReLU (decoder.6/7, networks.py:2253-2254) with the 6 x 6 x 10 input halo of a 4 x 4 x 8 block of INPUT
 * voxels in LDS and all eight output-parity classes computed from it (csrc/conv3d_halo.hip: convT3d_halo_kernel): in fp16 [B][d][h][w][cin],
 * out fp16 [B][2d][2h][2w][cout].  w8[4 pz + 2 py + px] = that class's fp16 [cout][8 * cin] matrix, K column (tz * 2 + tz... tap t) * cin + c
 * with t = (tz * 2 + ty) * 2 + tx, tap t_axis of parity p_axis reading input offset p - t (kernel index 1 + 2 t - p ... i.e. o = 2 i - 1 + k:
 * parity 0 -> k = 1, 3 at offsets 0, -1; parity 1 -> k = 0, 2 at offsets +1, 0) -- the layout pcd_vae_convT_t carries.  Supported:
 * cin 128, cout 64, dims multiples of (4, 4, 8); pcd_convt3d_k4s2_halo_supported() tells (1 / 0), unsupported -> PCD_ERR_ARG.
 * Same sums as the eight pcd_conv3d_f16 class launches in another order (fp32 accumulation; exact on integer operands). */
int pcd_convt3d_k4s2_halo_supported(int batch, int d, int h, int w, int cin, int cout);
int pcd_convt3d_k4s2_halo_f16(const void* in, int batch, int d, int h, int w, int cin, const void* const* w8, const float* bias,
                              int cout, void* out, void* stream);
/* encoder.0: Conv3d(1, cout, k3, stride 1|2, p1) (+ folded BN) + ReLU straight from the fp32 occupancy
 * grid x [B][D][H][W]; w fp32 [cout][27], out fp16 NDHWC (VAE3DLarge networks.py:2226, VAE3D :1999). */
int pcd_conv3d_first(const float* x, int batch, int d, int h, int w, int stride, const float* wgt,
                     const float* bias, int cout, void* out, void* stream);
/* decoder.12 + decoder.13: Conv3d(32, 1, k3, p1) + Sigmoid -> fp32 [B][D][H][W]; w fp32 [27][cin]. */
int pcd_conv3d_last_sigmoid(const void* in, int batch, int d, int h, int w, int cin, const float* wgt,
                            float bias, float* out, void* stream);
/* the same layer on the matrix pipe: wfrag = pcd_conv3d_last_pack's copy of wgt (pcd_conv3d_last_packed_bytes() bytes: the fp32 weights as fp16 hi / lo / lo2 rows of
 * the MFMA A operand of every tap); d, h, w multiples of 8, otherwise (or wfrag NULL, or pcd_conv3d_config + 8 / + 16) pcd_conv3d_last_sigmoid's kernels run from wgt */
size_t pcd_conv3d_last_packed_bytes(void);
int pcd_conv3d_last_pack(const float* wgt, void* wfrag, void* stream);
int pcd_conv3d_last_sigmoid_packed(const void* in, int batch, int d, int h, int w, int cin, const float* wgt, const void* wfrag, float bias, float* out,
                                   void* stream);
/* VAE3D's last layer (networks.py:2018-2019): ConvTranspose3d(32, 1, k3, s2, p1, output_padding 1) + Sigmoid;
 * in fp16 NDHWC [B][d][h][w][32], w fp32 [27][32] tap-major, out fp32 [B][2d][2h][2w]. */
int pcd_convt3d_last_sigmoid(const void* in, int batch, int d, int h, int w, int cin, const float* wgt,
                             float bias, float* out, void* stream);
/* z = mu + eps * exp(0.5 * logvar)  (networks.py:2323-2325), fp32 */
int pcd_reparameterize(const float* mu, const float* logvar, const float* eps, float* z, int64_t n, void* stream);

/* ---- whole VAE3DLarge.encode / decode (networks.py:2299-2310, 2327-2339) behind a handle ----
 * The host packer folds eval-mode BatchNorm3d into the conv weights and lays them out as the layer-level entry
 * points above expect: Conv3d [cout][k^3 * cin] tap-major zero-padded to kpad; each ConvTranspose3d(k4,s2,p1) as 8
 * output-parity classes [cout][8 * cin] with their 2x2x2 tap tables (class index = 4 pz + 2 py + px). */
typedef struct { const void* w; const float* b; int kpad, cin, cout, k; } pcd_vae_conv_t;
/* ResidualBlock3D.  fused_ds (with has_ds): c2 is [conv2 | downsample] -- kpad >= 27*c2.cin + ds.cin, the shortcut's folded weights in the
 * K columns behind the 27 taps, c2.b = b2 + b_ds -- and the block runs as two launches (pcd_conv3d_desc_t.in2); ds.cin / ds.cout describe
 * the shortcut, ds.w / ds.b are not read. */
typedef struct { pcd_vae_conv_t c1, c2, ds; int has_ds; int fused_ds; } pcd_vae_res_t;
typedef struct { const void* w[8]; const int* taps[8]; const float* b; int cin, cout; } pcd_vae_convT_t;
typedef struct {
    int latent_dim;
    const float* enc0_w; const float* enc0_b;          /* encoder.0 fp32 [32][27], [32] */
    pcd_vae_res_t enc_res[4];                          /* encoder.2, 5, 8, 11 */
    pcd_vae_conv_t enc_down[3];                        /* encoder.3, 6, 9   (k4, s2, p1) */
    pcd_vae_conv_t enc_last;                           /* encoder.12        (k4, p0) */
    const void* fc_w; const float* fc_b;               /* [fc_mu ; fc_logvar] fp16 [2*latent][512], fp32 [2*latent] */
    const void* din_w; const float* din_b;             /* decoder_input fp16 [512*64][latent], rows permuted to (z,y,x,c) */
    pcd_vae_convT_t dec_up[3];                         /* decoder.0, 3, 6 */
    pcd_vae_res_t dec_res[4];                          /* decoder.2, 5, 8, 11 */
    pcd_vae_conv_t dec_conv9;                          /* decoder.9 */
    const float* last_w; float last_b;                 /* decoder.12 fp32 [27][32] tap-major, bias */
    const int* taps3; const int* taps4s2; const int* taps4p0; const int* taps1;   /* regular tap tables (k3 p1, k4 p1, k4 p0, k1) */
    const void* zero_page;                             /* >= 128 bytes of zeros */
} pcd_vae_desc_t;
typedef struct pcd_vae pcd_vae_t;
int pcd_vae_create(const pcd_vae_desc_t* desc, pcd_vae_t** out);
/* Which layers of pcd_vae_encode / pcd_vae_decode leave the implicit GEMM / LDS-ring forms.  TEST / BENCHMARK ONLY: process-global.
 * PCD_ERR_ARG unless 0 <= code <= 15.
 *
 *   code         effect
 *   0            none of the three below
 *   1 (default)  all three (the same as 14)
 *   bit 1 (+ 2)  decoder.6 through pcd_convt3d_k4s2_halo_f16
 *   bit 2 (+ 4)  encoder.3 through pcd_conv3d_k4s2_halo_f16
 *   bit 3 (+ 8)  the k3 layers that have a fragment-order copy through pcd_conv3d_k3s1_wreg_f16
 *   bit 0 next to other bits is ignored */
int pcd_vae_config(int code);
void pcd_vae_destroy(pcd_vae_t* h);
size_t pcd_vae_workspace_bytes(int batch);
/* vox fp32 [B][1][32][32][32] in [0,1] -> mu_logvar fp32 [B][2*latent] = [mu | logvar] */
int pcd_vae_encode(pcd_vae_t* h, const float* vox, int batch, float* mu_logvar, void* workspace, size_t workspace_bytes,
                   void* stream);
/* z fp32 [B][latent] -> occupancy probabilities fp32 [B][1][32][32][32] */
int pcd_vae_decode(pcd_vae_t* h, const float* z, int batch, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* -------------------------------------------------------- set attention (K6/K7)
 * LayerNorm over C (eps 1e-5, biased var; networks.py:62,68) fp16 in -> fp16 out. */
int pcd_layernorm_f16(const void* x, int64_t rows, int c, const float* gamma, const float* beta,
                      void* out, void* stream);
/* softmax(Q K^T) V per (shape, head), flash style, never materialising N x N
 * (replaces the bmm/softmax/bmm path of nn.MultiheadAttention, networks.py:61,81).
 * qkv fp16 [B*N][3C] = [q | k | v] as produced by in_proj; q is scaled by 1/sqrt(d)
 * inside.  out fp16 [B*N][C] (heads concatenated, ready for out_proj).
 * V is transposed on the fly (ds_read_b64_tr_b16), so the workspace query returns 0 and
 * workspace may be NULL; the parameters are kept for ABI stability. */
size_t pcd_set_attention_workspace_bytes(int batch, int n_points, int c);
int pcd_set_attention_f16(const void* qkv, int batch, int n_points, int c, int heads,
                          void* out, void* workspace, size_t workspace_bytes, void* stream);
/* testing / tuning hook.  Dispatch: N % 256 == 0 selects the software-pipelined kernels (two 32-query blocks per wave: set_attention_sp_kernel at d = 64,
 * set_attention_spn_kernel at d = 32 / 16); every other length runs the one-block kernel with the same max-free softmax (set_attention_om_kernel).
 *   0 default; 1 = always the round-1 kernel (running max per tile); 2 = always the one-block max-free kernel;
 *   3 / 4 = d = 32 / 16 on the one-block kernel / on the pipelined kernel (default);
 *   5 / 6 = the d = 64 kernel as workgroups of four (default) / eight waves (same bits, measured equal);
 *   16 + bits = timing ablations of the pipelined kernels (1 no K/V restaging, 2 no rare-path test, 4 no waits / barriers): OUTPUTS ARE WRONG while set; 16 clears.
 * TEST / BENCHMARK ONLY: process-global. */
int pcd_set_attention_config(int force_generic);
/* name of the kernel the last pcd_set_attention_f16 call of this process launched (measurement reports quote it) */
const char* pcd_set_attention_last_kernel(void);
/* ---- training of the set-attention block (csrc/attn_bwd.hip; networks.py:51-83 under autograd).  n_points % 64 == 0.
 * Forward for training: pcd_set_attention_f16's output (the same kernels, the same bits) and lse fp32 [B][heads][N] =
 * ln sum_k exp(q . k / sqrt d) per query row (an exact second pass over the keys). */
int pcd_set_attention_lse_f16(const void* qkv, int batch, int n_points, int c, int heads, void* out, float* lse,
                              void* stream);
/* Backward of softmax(Q K^T / sqrt d) V, flash style (P recomputed from lse, the N x N matrix is never written):
 * qkv fp16 [B*N][3C] (the forward's input), out / dout fp16 [B*N][C], lse from pcd_set_attention_lse_f16 ->
 * dqkv fp16 [B*N][3C] = [dq | dk | dv] in qkv's layout, 1/sqrt(d) applied.  Deterministic: a key-block kernel (dK, dV)
 * and a query-block kernel (dQ) each own their output rows; no atomics.  workspace: fp32 delta = rowsum(dO o O). */
size_t pcd_set_attention_backward_workspace_bytes(int batch, int n_points, int c, int heads);
int pcd_set_attention_backward_f16(const void* qkv, const void* out, const void* dout, const float* lse, int batch,
                                   int n_points, int c, int heads, void* dqkv, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* LayerNorm for training, C = 64 / 128 / 256: the values of pcd_layernorm_f16, plus mean[rows] and rstd[rows] fp32 */
int pcd_layernorm_train_f16(const void* x, int64_t rows, int c, const float* gamma, const float* beta, void* out,
                            float* mean, float* rstd, void* stream);
/* its backward: dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) (added onto dx if accumulate; dx != dy), and
 * dgamma / dbeta [c] summed over all rows in a fixed order (per-workgroup slabs in the workspace, then one ordered sum) */
size_t pcd_layernorm_backward_workspace_bytes(int64_t rows, int c);
int pcd_layernorm_backward_f16(const void* dy, const void* x, int64_t rows, int c, const float* mean, const float* rstd,
                               const float* gamma, int accumulate, void* dx, float* dgamma, float* dbeta, void* workspace,
                               size_t workspace_bytes, void* stream);

/* x[m][c] + e[m / rows_per_shape][c] -> out (fp16 in/out, e fp32): the additive per-level time
 * embeddings of UNetAttentionPointExperimental (networks.py:669-698). */
int pcd_add_shape_bias_f16(const void* x, int64_t m, int c, int rows_per_shape, const float* e,
                           void* out, void* stream);
/* the same with the per-shape rows of e `e_stride` floats apart (0: one row shared by every shape) */
int pcd_add_shape_bias_strided_f16(const void* x, int64_t m, int c, int rows_per_shape, const float* e,
                                   int64_t e_stride, void* out, void* stream);
/* tail of UNetAttentionPointExperimental (networks.py:647-650,700-702): dec1 = PointNetLayer(128,3,3)
 * on cat[a | b] then Conv1d(3,3); BN folded.  w1 fp32 [3][ka+kb], w234 fp32 [3][3][3], b234 [3][3];
 * out fp32 [M][3]. */
int pcd_tail3(const void* a, int ka, const void* b, int kb, int64_t m, const float* w1, const float* b1,
              const float* w234, const float* b234, float* out, void* stream);

/* ---- whole SetAttentionBlock (networks.py:51-83) and UNetAttentionPointExperimental (networks.py:597-722) ----
 * Weights fp16 [C_out][C_in] (nn.Linear / in_proj layout), biases and LayerNorm affine fp32. */
typedef struct {
    int dim;                                         /* C: 64, 128 or 256 */
    const void* w_in;  const float* b_in;            /* attention.in_proj  [3C][C] */
    const void* w_out; const float* b_out;           /* attention.out_proj [C][C] */
    const float* ln1_g; const float* ln1_b; const float* ln2_g; const float* ln2_b;
    const void* w_ff1; const float* b_ff1;           /* ff.0 [4C][C] */
    const void* w_ff2; const float* b_ff2;           /* ff.2 [C][4C] */
    const void* ln_in_packed; const void* ln_ff1_packed;   /* optional (dim 256): pcd_pw_wide_ln_linear_pack images of (ln1, in_proj: 3 passes) and
                                                      * (ln2, ff.0: 4 passes): pcd_sab_forward then runs LN + Linear as one launch each when rows % 256 == 0 */
    const void* ffn_packed;                          /* optional (dim 256): pcd_wide_ffn_pack's image of ln2, ff.0, ff.2: LN2 + Linear + ReLU + Linear + residual as ONE launch
                                                      * (csrc/wideffn.hip; the 4C-wide hidden tensor is never written); rows % 128 == 0 */
    const void* tail_packed;                         /* optional (dim 64 / 128): pcd_sab_tail_pack's image of w_out .. b_ff2; pcd_sab_forward then runs
                                                      * out_proj + residual + LN2 + FFN + residual as ONE launch when rows % 256 == 0.  NULL: four launches.
                                                      * Ignored by the fp32 parity entry points */
} pcd_sab_desc_t;
/* The feed-forward half of the block at dim 256 as one launch (csrc/wideffn.hip; reference networks.py:62-68, 82):  y = x1 + W2 relu(W1 LN2(x1) + b1) + b2,
 * x1, y fp16 [rows][256] (y may not alias x1), rows % 128 == 0.  Two waves share 32 points and split the channels of both products, the 1024-wide hidden row lives in
 * registers / LDS 128 channels at a time, only the weights stream (pcd_wide_ffn_pack: 32 fragment-order stage images + b1 | b2 | gamma | beta,
 * pcd_wide_ffn_packed_bytes() bytes).  w1 [1024][256], w2 [256][1024] fp16; biases and the LayerNorm affine fp32. */
size_t pcd_wide_ffn_packed_bytes(void);
int pcd_wide_ffn_supported(int dim, int64_t rows);
int pcd_wide_ffn_pack(const void* w1, const float* b1, const void* w2, const float* b2, const float* ln_g, const float* ln_b, void* packed, void* stream);
int pcd_wide_ffn_f16(const void* packed, const void* x, int64_t rows, void* y, void* stream);
/* the same with the additive per-shape rows of networks.py:688 on the way out: y = fp16(y + post_e[row / rows_per_shape][c]) (fp32 rows of 256, e_stride floats
 * apart, 16-byte aligned; NULL = none) -- the rounding points of pcd_add_shape_bias_strided_f16 behind the block, bitwise the two launches */
int pcd_wide_ffn_bias_f16(const void* packed, const void* x, int64_t rows, int rows_per_shape, const float* post_e, int64_t e_stride, void* y, void* stream);
/* A/B hook (TEST / BENCHMARK ONLY, process-global): which waves request the weight images, see csrc/wideffn.hip; same bits either way */
int pcd_wide_ffn_config(int split);   /* 0 / 1 request form; 16 + bits = timing ablations of the kernel (OUTPUTS WRONG while set; 16 clears): TEST / BENCHMARK ONLY */
/* bytes of scratch one block needs for `rows` = B*N points */
size_t pcd_sab_workspace_bytes(int64_t rows, int dim);
/* the block's tail behind the attention kernel as one launch (csrc/sab_tail.hip; reference networks.py:78-83, the second half of SetAttentionBlock.forward):
 *   y = x1 + W2 relu(W1 LN2(x1) + b1) + b2,  x1 = x + W_out a + b_out      a = the heads' outputs [rows][dim], x = the block's input, all fp16
 * pcd_sab_tail_pack writes the fragment-order stage images of w_out / w_ff1 / w_ff2 (and w_in, for pcd_sab_head_f16) and the fp32 biases / LayerNorm affine of `d` into `packed`
 * (pcd_sab_tail_packed_bytes(dim) bytes of device memory; 0 = dim not supported); pcd_sab_tail_supported: dim 64 or 128 and rows % 256 == 0.
 * pcd_sab_tail_config(0) makes pcd_sab_forward / pcd_attn_unet_forward keep the four launches (A/B, tests); + 2: the fused launches with every wave requesting its
 * share of a stage's LDS-DMA pieces instead of one wave per SIMD (A/B); pcd_sab_tail_enabled reads bit 0 back.  TEST / BENCHMARK ONLY: process-global. */
size_t pcd_sab_tail_packed_bytes(int dim);
int pcd_sab_tail_supported(int dim, int64_t rows);
int pcd_sab_tail_pack(const pcd_sab_desc_t* d, void* packed, void* stream);
int pcd_sab_tail_f16(int dim, const void* packed, const void* a, const void* x, int64_t rows, void* y, void* stream);
/* the block's head in the same form, from the same image: qkv [rows][3 dim] = in_proj(LN1(x)) (networks.py:81), one launch instead of LayerNorm + GEMM */
int pcd_sab_head_f16(int dim, const void* packed, const void* x, int64_t rows, void* qkv, void* stream);
/* both with the attention U-Net's additive per-level time embeddings (networks.py:669-698) folded in: x is read as fp16(x + pre_e[row / rows_per_shape]) and
 * y leaves as fp16(y + post_e[row / rows_per_shape]), each rounded exactly as pcd_add_shape_bias_strided_f16 rounds it; pre_e / post_e fp32, rows e_stride
 * floats apart (0: one row for every shape; a multiple of 4), 16-byte aligned, either may be NULL */
int pcd_sab_tail_bias_f16(int dim, const void* packed, const void* a, const void* x, int64_t rows, int rows_per_shape, const float* pre_e,
                          const float* post_e, int64_t e_stride, void* y, void* stream);
int pcd_sab_head_bias_f16(int dim, const void* packed, const void* x, int64_t rows, int rows_per_shape, const float* pre_e, int64_t e_stride,
                          void* qkv, void* stream);
int pcd_sab_tail_config(int fused);
int pcd_sab_tail_enabled(void);
/* y = x + MHA(LN1 x); y = y + W2 relu(W1 LN2 y)   x, y fp16 [B*N][C], y must not alias x */
int pcd_sab_forward(const pcd_sab_desc_t* d, const void* x, int batch, int n_points, int heads, void* y,
                    void* workspace, size_t workspace_bytes, void* stream);

#define PCD_ATTN_UNET_NLIN 14       /* enc1.conv2,3  enc2.conv1-3  enc3.conv1-3  dec3.conv1-3  dec2.conv1-3 (BN folded) */
#define PCD_ATTN_UNET_NSAB 7        /* att1 att2 att3 bottleneck att_dec3 att_dec2 att_dec1 */
#define PCD_ATTN_UNET_NEMB 6        /* emb1 emb2 emb3 emb_dec3 emb_dec2 emb_dec1 */
#define PCD_ATTN_UNET_TB 704        /* floats of one time-bias row: [enc1 bias 64 | emb2 64 | emb3 128 | emb_dec3 256 | emb_dec2 128 | emb_dec1 64] */
typedef struct {
    int dim, time_dim, heads;
    const float* freqs;                              /* sinusoidal frequencies [time_dim/2] */
    const float* tw0; const float* tb0; const float* tw2; const float* tb2;    /* time_mlp */
    const float* emb_w[PCD_ATTN_UNET_NEMB]; const float* emb_b[PCD_ATTN_UNET_NEMB];   /* [c][dim], c = 3,64,128,256,128,64 */
    const float* e1w; const float* e1b;              /* enc1.conv1 + bn1 folded, fp32 [64][3], [64] */
    pcd_linear_desc_t lin[PCD_ATTN_UNET_NLIN];
    pcd_sab_desc_t sab[PCD_ATTN_UNET_NSAB];
    const float* t_w1; const float* t_b1; const float* t_w234; const float* t_b234;   /* dec1 + output, see pcd_tail3 */
} pcd_attn_unet_desc_t;
typedef struct pcd_attn_unet pcd_attn_unet_t;
int pcd_attn_unet_create(const pcd_attn_unet_desc_t* desc, pcd_attn_unet_t** out);
void pcd_attn_unet_destroy(pcd_attn_unet_t* h);
size_t pcd_attn_unet_workspace_bytes(int batch, int n_points);
/* time path for n_t values of t: tbias fp32 [n_t][PCD_ATTN_UNET_TB] (time_mlp, the six emb* layers, and emb1 pushed
 * through enc1.conv1: conv(x + e) = W x + (W e + b), networks.py:664-672); scratch fp32 [n_t][dim] */
int pcd_attn_unet_time_bias(pcd_attn_unet_t* h, const float* t, int n_t, float* scratch, float* tbias, void* stream);
/* eps = model(x, t) given the time-bias rows: tbias row (b * tbias_shape_stride), stride 0 = one t for every shape */
int pcd_attn_unet_forward(pcd_attn_unet_t* h, const float* x, int batch, int n_points, const float* tbias,
                          int tbias_shape_stride, float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* parity taps of the last forward: "x1" [B*N][64], "x2" [B*N][128], "x3" [B*N][256] fp16 (the skip tensors, networks.py:663-672) */
int pcd_attn_unet_tap(pcd_attn_unet_t* h, const char* name, int batch, int n_points, const void* workspace, void* dst,
                      size_t dst_bytes, void* stream);

/* ------------------------------------------------ fp32 parity mode of the set-attention block and the attention U-Net (csrc/attn_f32.hip)
 * pcd_sab_forward / pcd_attn_unet_forward with fp32 weights (EVERY weight pointer of the descriptors is fp32 here), fp32 activations and
 * fp32 arithmetic (pcd_gemm_f32, fp32 LayerNorm, a plain fp32 softmax(q k^T / sqrt d) v kernel): the reference's arithmetic type
 * (networks.py:51-83, 597-722), held to 1e-4.  x / y / eps fp32; tbias = the 704-float rows of pcd_attn_unet_time_bias (fp32 in both modes).
 * Taps of the last forward: x1 / x2 / x3, fp32. */
size_t pcd_sab_f32_workspace_bytes(int64_t rows, int dim);
int pcd_sab_f32_forward(const pcd_sab_desc_t* d, const float* x, int batch, int n_points, int heads, float* y, void* workspace,
                        size_t workspace_bytes, void* stream);
typedef struct pcd_attn_unet_f32 pcd_attn_unet_f32_t;
int pcd_attn_unet_f32_create(const pcd_attn_unet_desc_t* desc, pcd_attn_unet_f32_t** out);
void pcd_attn_unet_f32_destroy(pcd_attn_unet_f32_t* h);
size_t pcd_attn_unet_f32_workspace_bytes(int batch, int n_points);
int pcd_attn_unet_f32_forward(pcd_attn_unet_f32_t* h, const float* x, int batch, int n_points, const float* tbias,
                              int tbias_shape_stride, float* eps, void* workspace, size_t workspace_bytes, void* stream);
int pcd_attn_unet_f32_tap(pcd_attn_unet_f32_t* h, const char* name, int batch, int n_points, const void* workspace, void* dst,
                          size_t dst_bytes, void* stream);

/* ------------------------------------------------------------- metrics (K10-K12)
 * normalize_to_cube (metrics.py:7-21) for B clouds of N points, fp32 in/out. */
int pcd_normalize_to_cube(const float* pts, int batch, int n, float* out, void* stream);
/* Chamfer sums (metrics.py:41-46) on already-normalised clouds:
 * sums[b][0] = sum_i min_j |x_i - y_j|, sums[b][1] = sum_j min_i |x_i - y_j| (unsquared L2),
 * direct differences in fp32 (no matmul cancellation).  sums fp32 [B][2]. */
int pcd_chamfer_sums(const float* x, const float* y, int batch, int n1, int n2, float* sums, void* stream);
/* voxelize (utils.py:488-509): occupancy fp32 [B][R][R][R] indexed [x][y][z]; caller zeroes out. */
int pcd_voxelize(const float* pts, int batch, int n, int res, float* vox, void* stream);
/* voxel_tensor_to_point_clouds (utils.py:511-539): for each grid (D,H,W) emit the points with
 * v > threshold in row-major (z,y,x) order as [x,y,z] mapped to [-1,1].
 * counts int32 [B]; points fp32 [B][D*H*W][3] (first counts[b] rows valid). */
int pcd_voxels_to_points(const float* vox, int batch, int d, int h, int w, float threshold,
                         int32_t* counts, float* points, void* stream);
/* mean BCE(x, target) with torch's log clamp at -100 (metrics.py:181); out fp32 [1]. */
int pcd_binary_bce_mean(const float* x, const float* target, int64_t n, float* out, void* stream);

/* ---- Surface-nets meshes of occupancy grids (csrc/mesh.hip; definition in DESIGN.md "Mesh output") ----
 * vox fp32 [B][D][H][W] as pcd_voxels_to_points reads it, any d, h, w > 1; a node is inside iff v > threshold, 0 < threshold < inf.
 * The field is surrounded by one layer of nodes of value 0, so every mesh is closed.  Cell (cz, cy, cx), 0 <= cz <= D (likewise cy, cx),
 * has the padded nodes (cz + a, cy + b, cx + c), a, b, c in {0, 1}; a cell whose corners are not all on one side owns one vertex, the mean
 * of the crossing points A + (threshold - v_A) / (v_B - v_A) (B - A) of its edges whose ends differ in side.  Vertices are numbered in row-major
 * (cz, cy, cx) order and leave as [x, y, z] rows under the affine map of pcd_voxels_to_points (index i of an axis of n nodes -> 2 i / (n - 1) - 1;
 * surfaces that close in the padding reach up to one pitch 2 / (n - 1) outside [-1, 1]).  Faces: per padded node in row-major order and per axis
 * z, y, x, the edge to the +1 neighbour, where its ends differ in side, gives one quad of the four cells round it, as two triangles
 * (q0, q1, q2), (q0, q2, q3), wound so that normals point outward.  One workgroup per grid, ballot + block-scan compaction, no atomics: bitwise
 * repeatable and independent of the rest of the batch.
 *
 * Two calls with one host read of `counts` between them to size the packed outputs:
 *   pcd_mesh_count  leaves in `workspace` each cell's vertex number or -1 -- int32 [B][D+1][H+1][W+1], pcd_mesh_workspace_bytes() bytes (host
 *                   arithmetic; 0 for arguments the other two refuse) -- and counts int32 [B][2] = (vertices, triangles) of each grid.
 *   pcd_mesh_emit   with the same vox, extents, threshold and workspace: offsets int64 [B][2] = first vertex row, first face row of each grid
 *                   (the exclusive running sums of counts); vertices fp32 [sum V][3]; faces int32 [sum F][3], indices local to the grid.
 * V <= (D+1)(H+1)(W+1), F <= 2 ((W+1)HD + (H+1)DW + (D+1)HW).  PCD_ERR_ARG (before any device work) for a null pointer, batch <= 0, an extent
 * <= 1, a threshold <= 0 or not finite, or more than (2^31 - 1) / 6 cells per grid. */
size_t pcd_mesh_workspace_bytes(int batch, int d, int h, int w);
int pcd_mesh_count(const float* vox, int batch, int d, int h, int w, float threshold, void* workspace, int32_t* counts, void* stream);
int pcd_mesh_emit(const float* vox, int batch, int d, int h, int w, float threshold, const void* workspace, const int64_t* offsets,
                  float* vertices, int32_t* faces, void* stream);
/* Which form the two mesh kernels take.  TEST / BENCHMARK ONLY: process-global.  1 (default): a grid of at most 144 KB is staged in LDS once
 * per workgroup and the corner reads are served from there; 0: every grid is read through the vector cache, as larger grids always are.
 * Same bits either way.  PCD_ERR_ARG for any other code. */
int pcd_mesh_config(int code);

/* ---- Triangle meshes in: voxelizer and surface sampler (csrc/mesh_in.hip; DESIGN.md "Mesh input") ----
 * A batch of meshes is packed as pcd_mesh_emit packs its outputs: vertices fp32 [sum V][3] rows [x, y, z]; faces int32 [sum F][3], indices
 * local to the mesh; offsets int64 [B + 1][2] = first vertex row, first face row of each mesh, the totals in the last row.  A face with an
 * index outside its mesh's rows is skipped (it marks nothing, has area 0).
 *
 * Voxelizer.  All index work is done in index coordinates p = (x - lo) * inv_pitch per component, inv_pitch = (R - 1) / (hi - lo) computed by the
 * caller in double and passed as fp32: node i of an axis sits at p = i, which for bounds (-1, 1) inverts the 2 i / (R - 1) - 1 map of
 * pcd_voxels_to_points / pcd_mesh_emit.  vox fp32 [B][R][R][R] indexed [z][y][x], values 0 or 1.
 *   Surface   node (z, y, x) is 1 iff some triangle of the mesh intersects the closed cube of side 1 centred on the node: triangle / box overlap by
 *             the 13 separating axes -- the 3 box normals, the triangle normal n = (b - a) x (c - a), and e x X, e x Y, e x Z for the edges
 *             e = b - a, c - b, a - c.  With the vertices taken relative to the node, an axis separates iff the least projection of the three
 *             vertices exceeds the cube's radius 1/2 (|l_x| + |l_y| + |l_z|) on that axis l, or the greatest is below its negative; touching
 *             counts as intersecting.  A triangle of zero area is tested as the segment or point it is (its zero axes separate nothing).
 *   Interior  for node (z, y, x) take every triangle whose projection on the xy plane covers the point (y, x): exact edge functions
 *             E(p, q) = p_x q_y - p_y q_x of the vertices relative to the point, after orienting the projection counter-clockwise (b and c are
 *             swapped when n_z < 0), covered iff all three are > 0 or, where one is 0, its edge is a top-left one: d_y < 0, or d_y = 0 and
 *             d_x > 0, for d = q - p (the point is sampled at (x + eps, y + eps^2)).  Triangles with n_z = 0 contribute nothing.  With z* the
 *             height of the triangle's plane over (y, x), the winding of the node is the sum of sign(n_z) over those triangles with z* > z
 *             (strictly), decided without division as sign(n_z) n . (a - p) > 0, p the node.  The node is 1 iff the winding is not 0 (nonzero
 *             winding, not parity: overlapping closed components fill as one solid, an inside-out one fills too).
 *   Solid     the union of the two.
 * The predicates are fp32 without contraction: on inputs whose intermediate values are exactly representable they decide ties as this statement
 * does.  Integer atomics only, one workgroup per mesh, no host synchronisation: bitwise repeatable and independent of the rest of the batch.  A
 * mesh without faces gives an all-zero grid.  workspace: pcd_mesh_voxelize_workspace_bytes() bytes (host arithmetic, 0 for arguments
 * pcd_mesh_voxelize refuses), any contents; the accumulators of a grid with R > 32 live there, smaller ones in LDS.
 * PCD_ERR_ARG (before any device work) for a null pointer, batch <= 0, r < 2 or r > 64, an unknown mode, a non-finite lo or inv_pitch, or
 * inv_pitch <= 0. */
#define PCD_MESH_FILL_SURFACE 0
#define PCD_MESH_FILL_INTERIOR 1
#define PCD_MESH_FILL_SOLID 2
size_t pcd_mesh_voxelize_workspace_bytes(int batch, int r);
int pcd_mesh_voxelize(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int r, float lo, float inv_pitch,
                      int mode, void* workspace, float* vox, void* stream);
/* Sampler: points fp32 [B][N][3] uniform by area on each mesh's surface, in the vertices' own coordinates.  Two launches:
 *   1. triangle areas |e0 x e1| / 2 in fp32 and, per mesh, their inclusive running sum, left in the workspace (fp32 [sum F],
 *      pcd_mesh_sample_workspace_bytes() bytes); added in a fixed tree (lanes of a wave, the 16 waves, then chunks of 1024 faces in order), so the
 *      same input gives the same bits.  A face whose area is not finite counts as 0.
 *   2. per output point i of mesh b three uniforms u0, u1, u2 in [0, 1): u[b][i][0..2] when u (fp32 [B][N][3]) is not null, otherwise from
 *      Philox4x32-10 as in pcd_randn -- counter words {lo(ctr), hi(ctr), 0, 0}, key {lo(seed), hi(seed)} -- with ctr = philox_offset + i and
 *      u_k = (word k >> 8) / 2^24 (word 3 is not used).  The counter does not depend on b: a mesh gets in a batch the bits it gets alone, and
 *      a call consumes the counters [philox_offset, philox_offset + N).  Triangle f is the first whose running sum exceeds u0 * total (the
 *      last one at most); the point is (1 - s) A + s (1 - u2) B + s u2 C with s = sqrt(u1).
 * normals (optional, fp32 [B][N][3]): the unit face normal (b - a) x (c - a) / |.|, zero for a zero-area face.  face_index (optional, int32
 * [B][N]): f, local to the mesh.  A mesh whose total area is 0 puts every point on the first vertex of its first face; a mesh without faces
 * gives zero rows (callers refuse them on the host, where offsets is built).  PCD_ERR_ARG for a null vertices, faces, offsets, workspace or
 * points, batch <= 0 or > 65535, n_points <= 0. */
size_t pcd_mesh_sample_workspace_bytes(int batch, int64_t total_faces);
int pcd_mesh_sample_points(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int n_points, uint64_t seed,
                           uint64_t philox_offset, const float* u, void* workspace, float* points, float* normals, int32_t* face_index,
                           void* stream);

/* ---- Mesh processing: vertex rings, smoothing, normals, components, compaction, measures (csrc/mesh_ops.hip; DESIGN.md "Mesh processing") ----
 * Meshes are packed as for pcd_mesh_voxelize: vertices fp32 [sum V][3], faces int32 [sum F][3] local to the mesh, offsets int64 [B + 1][2].
 * total_vertices and total_faces are the last row of offsets, known to the caller on the host (rows past them are never read); max_vertices
 * (pcd_mesh_components) is an upper bound of every mesh's V (total_vertices is one) and only decides which launches are made.  A face is VALID iff its three indices
 * are rows of its mesh and pairwise different; every function skips the others.  No floating-point atomics, every sum in a fixed order, every
 * device loop bounded by V, F or the iteration count: bitwise repeatable, a mesh gets in a batch what it gets alone, and empty meshes are legal.
 * No host synchronisation except between pcd_mesh_compact_count and pcd_mesh_compact_emit.  PCD_ERR_ARG (before any device work) for a null
 * pointer, batch outside 1 .. 65535, total_vertices >= 2^31 - 1, 6 total_faces >= 2^31 - 1024, or max_vertices > total_vertices.
 *
 * Adjacency.  Rows are indexed by packed vertex row g (nbr_start, inc_start int32 [sum V + 1], exclusive running sums by a device scan; the sizes
 * are bounded by 6 and 3 entries per face, so nothing is sized from the data).  Row g of nbr_index (int32 [6 sum F]) holds the distinct
 * neighbours u of the vertex (local indices, they share an edge of a valid face) in ascending u, and nbr_counts (int32 [6 sum F][2]) per entry
 * (out, in) = the number of valid faces holding the directed edge a -> u and u -> a.  Row g of inc_faces (int32 [3 sum F]) holds its incident valid
 * faces (local) in ascending order.  Entries past nbr_start[sum V] / inc_start[sum V] are not written.  flags int32 [sum V]:
 * PCD_MESH_VERTEX_REFERENCED (in some valid face), _BOUNDARY (some entry has out + in == 1), _IRREGULAR (some entry has out != 1 or in != 1: a
 * boundary, a non-manifold edge or an inconsistently oriented one).  Rows of any length (one wave sorts a row by rank). */
#define PCD_MESH_VERTEX_REFERENCED 1
#define PCD_MESH_VERTEX_BOUNDARY 2
#define PCD_MESH_VERTEX_IRREGULAR 4
size_t pcd_mesh_adjacency_workspace_bytes(int batch, int64_t total_vertices, int64_t total_faces);
int pcd_mesh_adjacency(const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices, int64_t total_faces, void* workspace,
                       int32_t* nbr_start, int32_t* nbr_index, int32_t* nbr_counts, int32_t* inc_start, int32_t* inc_faces, int32_t* flags,
                       void* stream);
/* Taubin smoothing: `iterations` rounds of a lam step then (mu != 0) a mu step of the uniform umbrella operator, Jacobi style.  Per step and
 * component, fp32 without contraction: s = +0; s = s + x[u] over the row in order; m = s / float(n); x' = x + f (m - x).  A vertex with an empty
 * row keeps its position, with pin_boundary a BOUNDARY vertex does too, bitwise.  One launch per step over the whole batch, one thread per
 * vertex, the positions alternating between `workspace` (pcd_mesh_smooth_workspace_bytes()) and out so that the last step lands in out.
 * out fp32 [sum V][3], not `vertices`.  PCD_ERR_ARG also for iterations outside 0 .. 2^20, lam outside (0, 1], mu outside (-1, 0] or a factor
 * that is not finite. */
size_t pcd_mesh_smooth_workspace_bytes(int64_t total_vertices);
int pcd_mesh_smooth(const float* vertices, const int64_t* offsets, int batch, int64_t total_vertices, const int32_t* nbr_start,
                    const int32_t* nbr_index, const int32_t* flags, int iterations, float lam, float mu, int pin_boundary, void* workspace,
                    float* out, void* stream);
/* Area-weighted vertex normals, fp32 without contraction: per incident face in ascending order e1 = b - a, e2 = c - a (a, b, c in the face's
 * order), n += (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) from +0; len = sqrt((nx nx + ny ny) + nz nz); normals fp32 [sum V][3] =
 * n / len, zeros where len is 0 or the vertex is unreferenced. */
int pcd_mesh_vertex_normals(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                            const int32_t* inc_start, const int32_t* inc_faces, float* normals, void* stream);
/* Connected components by min-label propagation with pointer jumping, one workgroup per mesh, at most V sweeps.  labels int32 [sum V]: the
 * least vertex index of the component, -1 for an unreferenced vertex; counts int32 [B]: components per mesh; component_faces int32 [sum V]: at a
 * label root the valid faces of its component, 0 elsewhere.  Labels of a mesh of at most PCD_MESH_LABELS_LDS_MAX_V vertices live in LDS while
 * they move, larger ones in `workspace` (pcd_mesh_components_workspace_bytes()). */
#define PCD_MESH_LABELS_LDS_MAX_V 32768
size_t pcd_mesh_components_workspace_bytes(int64_t total_vertices);
int pcd_mesh_components(const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices, int64_t max_vertices,
                        const int32_t* nbr_start, const int32_t* nbr_index, const int32_t* flags, void* workspace, int32_t* labels,
                        int32_t* counts, int32_t* component_faces, void* stream);
/* keep int32 [sum V] = 1 for the vertices of the chosen components, 0 elsewhere (unreferenced vertices always 0).  PCD_MESH_KEEP_LARGEST: the
 * component with the most faces, the smaller label on a tie; PCD_MESH_KEEP_MIN_FACES: every component with at least min_faces (>= 0) faces. */
#define PCD_MESH_KEEP_LARGEST 0
#define PCD_MESH_KEEP_MIN_FACES 1
int pcd_mesh_component_keep(const int64_t* offsets, int batch, const int32_t* labels, const int32_t* component_faces, int rule, int min_faces,
                            int32_t* keep, void* stream);
/* Compaction under keep int32 [sum V] (nonzero = kept): the kept vertices in order, and in order the valid faces whose three vertices are all
 * kept, renumbered.  The protocol of pcd_mesh_count / pcd_mesh_emit: pcd_mesh_compact_count leaves each vertex's new index or -1 in `workspace`
 * (pcd_mesh_compact_workspace_bytes()) and counts int32 [B][2] = (vertices, faces); the caller sizes the outputs on the host and passes
 * out_offsets int64 [B][2], the exclusive running sums of counts, to pcd_mesh_compact_emit with the same inputs and workspace. */
size_t pcd_mesh_compact_workspace_bytes(int64_t total_vertices);
int pcd_mesh_compact_count(const int32_t* faces, const int64_t* offsets, int batch, const int32_t* keep, void* workspace, int32_t* counts,
                           void* stream);
int pcd_mesh_compact_emit(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const void* workspace,
                          const int64_t* out_offsets, float* out_vertices, int32_t* out_faces, void* stream);
/* Measures.  real float64 [B][5] = area sum |e1 x e2| / 2, signed volume sum a . (b x c) / 6, and the area-weighted centroid of the surface
 * (zeros for area 0), formed per face in double from the fp32 vertices and added in a fixed tree (the butterfly of a wave, the 16 waves in order,
 * then chunks of 1024 faces in order).  whole int32 [B][8] = referenced vertices, undirected edges (ring entries / 2), valid faces, boundary
 * edges (out + in == 1), irregular edges (out != 1 or in != 1), components (the roots of `labels` from pcd_mesh_components), the Euler
 * characteristic V - E + F of those three, and closed = 1 iff every entry has out == in. */
int pcd_mesh_measures(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const int32_t* nbr_start,
                      const int32_t* nbr_index, const int32_t* nbr_counts, const int32_t* labels, double* real, int32_t* whole, void* stream);
/* Where pcd_mesh_components keeps the moving labels.  TEST ONLY: process-global.  0 (default): in LDS for the meshes they fit; 1: always in
 * the workspace, as for larger meshes.  Same bits either way.  PCD_ERR_ARG for any other code. */
int pcd_mesh_ops_config(int code);

/* ---- Mesh simplification: vertex clustering with quadric-optimal representatives (csrc/mesh_simplify.hip; DESIGN.md "Mesh simplification") ----
 * Packing, valid faces and the promises (integer atomics only, fixed-order sums, bounded loops, bitwise repeatable, a mesh gets in a batch what
 * it gets alone, empty meshes legal) as in the block above.  Per mesh a cubic grid of R^3 cells of side h over the box of the referenced
 * vertices; the referenced vertices of a cell form a cluster, numbered by their least vertex index; a valid face survives iff its three
 * clusters differ (and, with `deduplicate`, iff it is the first with its oriented triple of clusters up to rotation); a cluster's vertex is
 * the regularised minimiser of its summed face quadrics (PCD_MESH_SIMPLIFY_QUADRIC) or the mean of its members (_MEAN), in fp64, rounded to fp32.
 *
 * `params` is a device array of one entry per mesh, read by `mode`: _RESOLUTION int32 R (h = ext / R), _CELL_SIZE fp32 h (R follows from the
 * box), _TARGET_FACES int32 face budget (ten rounds of bisection over R in 1 .. 1024 on the device, surviving faces <= budget).  The entries
 * are the caller's to validate (shapegen_amd.mesh_ops does); the kernels clamp R to 1 .. PCD_MESH_SIMPLIFY_MAX_RESOLUTION, take R = 1 for a
 * cell size that is not finite and positive, and a negative budget as 0, so no entry can index out of range.
 *
 * The protocol of pcd_mesh_compact_count / _emit: pcd_mesh_simplify_count writes resolutions int32 [B] (the R used), map int32 [sum V] (vertex ->
 * cluster number of its mesh, -1 unreferenced) and counts int32 [B][2] = (clusters, surviving faces); the caller sizes the outputs on the host
 * -- the one host read -- and passes out_offsets int64 [B][2], the exclusive running sums of counts, to pcd_mesh_simplify_emit with the same
 * inputs and the workspace as _count left it.  max_vertices is an upper bound of every mesh's V.  PCD_ERR_ARG (nothing launched) for a null
 * pointer, an unknown mode, placement or deduplicate flag, sizes the block above refuses, max_vertices > total_vertices or
 * max_vertices >= PCD_MESH_SIMPLIFY_MAX_VERTICES; PCD_ERR_WORKSPACE for workspace_bytes below pcd_mesh_simplify_workspace_bytes() (0 = refused sizes). */
#define PCD_MESH_SIMPLIFY_RESOLUTION 0
#define PCD_MESH_SIMPLIFY_CELL_SIZE 1
#define PCD_MESH_SIMPLIFY_TARGET_FACES 2
#define PCD_MESH_SIMPLIFY_QUADRIC 0
#define PCD_MESH_SIMPLIFY_MEAN 1
#define PCD_MESH_SIMPLIFY_MAX_RESOLUTION 1024
#define PCD_MESH_SIMPLIFY_MAX_VERTICES (1 << 21)
size_t pcd_mesh_simplify_workspace_bytes(int batch, int64_t total_vertices, int64_t total_faces);
int pcd_mesh_simplify_count(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                            int64_t total_faces, int64_t max_vertices, int mode, const void* params, int deduplicate, void* workspace,
                            size_t workspace_bytes, int32_t* resolutions, int32_t* map, int32_t* counts, void* stream);
int pcd_mesh_simplify_emit(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, int64_t total_vertices,
                           int64_t total_faces, int64_t max_vertices, int placement, void* workspace, size_t workspace_bytes,
                           const int64_t* out_offsets, float* out_vertices, int32_t* out_faces, void* stream);

/* ---- Images out: depth-buffered renderer for point clouds and triangle meshes (csrc/render.hip; DESIGN.md "Render") ----
 * View.  views fp32 [view_sets][V][12], a row-major 3 x 4 matrix [M | t] each; view_sets = 1 shares the V views among the shapes, view_sets = B
 * gives every shape its own.  A world point p maps to q = M p + t = (x, y, z), each component evaluated in fp32 without contraction as
 * ((m0 px + m1 py) + m2 pz) + t: x, y in pixels (x right, y down, the centre of pixel (i, j) at (j + 1/2, i + 1/2)), z the depth in pixel
 * units, smaller = nearer.  Orthographic only.  A primitive with a projected coordinate that is not finite is skipped.
 *   Points     pcd_render_points: points fp32 [sum n][3], offsets int64 [B + 1] = first row of each cloud, the total last.  Point k covers the
 *              pixel centre c iff dx^2 + dy^2 <= r^2 with (dx, dy) = c - (qx, qy) (evaluated (dx dx + dy dy) <= r r); depth qz on the whole
 *              disc; shading normal n = (dx, dy, -sqrt(r^2 - (dx^2 + dy^2))) / r, L = max(0, n . l).
 *   Triangles  pcd_render_meshes: packed as for pcd_mesh_voxelize (offsets int64 [B + 1][2]); a face with an index outside its mesh's rows is
 *              skipped; both faces are drawn.  With u = q1 - q0, v = q2 - q0 and n = u x v, a triangle with n_z = 0 (screen area 0) draws
 *              nothing.  Every edge is evaluated from its canonical order -- the endpoint A with the lexicographically smaller (x, y) first,
 *              d = B - A: e(c) = d_x (c_y - A_y) - d_y (c_x - A_x), and w = e(the third vertex) (w = 0: the triangle draws nothing).  With
 *              s = sign(w) and the inward normal (nx, ny) = s (-d_y, d_x) the centre is inside the edge iff s e > 0, or e = 0 and
 *              (nx > 0, or nx = 0 and ny > 0): the top-left rule.  Two triangles that share an edge evaluate the same e, so a closed mesh is
 *              watertight in fp32.  Depth z0 - (n_x (c_x - x0) + n_y (c_y - y0)) / n_z (a pixel where it is not finite is not covered);
 *              L = |n . l| / |n|.
 * Visibility: per pixel the covering primitive with the least (depth, index) wins; depth compared as fp32 (-0 = +0), equal depth to the lower
 * index; independent of the order of evaluation.  Outputs [B][V][H][W](,3), each optional (null: not written): ids int32 = the winner's row
 * local to its shape, -1 for background; depth fp32, +inf for background; rgb uint8 = floor(min(max((255 color_k) (ambient + (1 - ambient) L),
 * 0), 255) + 1/2), the background round(255 background_k).  One launch, one workgroup per (shape, view, tile of 128 x 64 or 128 x 128 pixels),
 * visibility keys in LDS, integer atomics only: bitwise repeatable, independent of the rest of the batch and of the tile shape; no workspace.
 * PCD_ERR_ARG (before any device work) for a null input or style, batch or n_views outside 1 .. 65535, view_sets not 1 or batch, height or
 * width outside 1 .. 2048, radius outside (0, 64] or an ambient outside [0, 1]. */
typedef struct {
    const float* colors;      /* fp32 [B][3] RGB in [0, 1] per shape, or null: (0.27, 0.51, 0.71) for all */
    float light[3];           /* l: unit vector in view space */
    float ambient;
    float background[3];      /* RGB in [0, 1] */
} pcd_render_style_t;
int pcd_render_points(const float* points, const int64_t* offsets, int batch, const float* views, int view_sets, int n_views, int height,
                      int width, float radius, const pcd_render_style_t* style, int32_t* ids, float* depth, uint8_t* rgb, void* stream);
int pcd_render_meshes(const float* vertices, const int32_t* faces, const int64_t* offsets, int batch, const float* views, int view_sets,
                      int n_views, int height, int width, const pcd_render_style_t* style, int32_t* ids, float* depth, uint8_t* rgb,
                      void* stream);
/* The tile of a workgroup.  TEST / BENCHMARK ONLY: process-global.  0: 128 x 64 pixels (64 KB of keys); 1: 128 x 128 (128 KB); 2 (default): 128 x 64
 * while that is at most one workgroup per CU, 128 x 128 for larger launches.  Same bits every way.  PCD_ERR_ARG for any other code. */
int pcd_render_config(int code);

/* ---- Sinkhorn EMD (metrics.py:94-158, `earth_mover_distance_gpu`), cost matrix never stored ----
 * out_max[0] = max over (b,i,j) of |x_i - y_j|   (the global C.max() of metrics.py:123) */
int pcd_pairwise_max_dist(const float* x, const float* y, int batch, int n, int m, float* out_max, void* stream);
/* one half-iteration (metrics.py:141 / :144): for the rows of p against cloud q with dual dual_q,
 * dual_p[i] <- epsilon * (log_marginal - logsumexp_j(-|p_i - q_j| / (cmax*epsilon) + dual_q[j]));
 * err_max[0] = max_i |new - old| (metrics.py:147-148).  duals fp32 [B][n]. */
int pcd_sinkhorn_dual_update(const float* p, const float* q, int batch, int np, int nq, const float* cmax,
                             float epsilon, float log_marginal, const float* dual_q, float* dual_p,
                             float* err_max, void* stream);
/* cost[b] = sum_ij exp(-C/eps + alpha_i + beta_j) * C_ij (metrics.py:153-156); row_scratch fp32 [B][n] */
int pcd_sinkhorn_cost(const float* x, const float* y, int batch, int n, int m, const float* cmax,
                      float epsilon, const float* alpha, const float* beta, float* row_scratch,
                      float* cost, void* stream);

/* ---- a batch of independent cloud pairs in one enqueue (the evaluation loop of test_point_ddpm.py:85-92) ----
 * Pair p = a[p][0..na[p]) vs b[p][0..nb[p]) inside padded fp32 arrays [P][na_max][3] / [P][nb_max][3]; na, nb device
 * int32 [P]; a pair with a count of 0 gets a NaN row (the reference's compute_metrics would raise on an empty cloud).  rows fp32 [P][3] = (Chamfer with scaling 1 (metrics.py:23-47), Sinkhorn EMD
 * (metrics.py:94-158, only when with_sinkhorn, else 0), voxel BCE (metrics.py:177-181)), each computed exactly as
 * compute_metrics(a_p, b_p) would for that pair alone: per-pair normalize_to_cube, per-pair cost normalisation, per-pair
 * convergence test (kept on the device: all max_iter iterations are enqueued, converged pairs skip theirs; no host
 * synchronisation).  log_mu[p] = log(1/na[p] + 1e-10), log_nu likewise, fp32 device arrays from the host's torch ops. */
size_t pcd_pair_metrics_workspace_bytes(int pairs, int na_max, int nb_max);
int pcd_pair_metrics(const float* a, const int* na, int na_max, const float* b, const int* nb, int nb_max, int pairs,
                     int with_sinkhorn, float epsilon, float thresh, int max_iter, const float* log_mu,
                     const float* log_nu, float* rows, void* workspace, size_t workspace_bytes, void* stream);
/* What pcd_pair_metrics leaves in its workspace, for callers that want the stages and not only the rows.  Fills
 * offsets[PCD_PAIR_WS_FIELDS] with byte offsets (each a multiple of 256) in this order, NQ = max(na_max, nb_max):
 *   AN, BN      the normalised clouds, fp32 [P][na_max][3] / [P][nb_max][3] (rows past a pair's count are not written)
 *   MINS        min_j |q - t_j|^2 per query, fp32 [P][2][NQ]: [p][0] queries a against b, [p][1] queries b against a
 *   ALPHA, BETA the duals after the last iteration the pair ran, fp32 [P][na_max] / [P][nb_max]
 *   ROWC        sum_j P_ij C_ij per row of a, fp32 [P][na_max] (rows[p][1] is its sum)
 *   CMAX        the pair's max_ij |a_i - b_j| of the normalised clouds, fp32 [P]
 *   ERR         the two error slots (alpha, beta) of both iteration parities, fp32 [2][P][2]: parity (max_iter - 1) & 1 holds what the
 *               last enqueued iteration left (its errors, or zeros for a pair that had stopped before it), the other parity is cleared
 *   BITS        the 32^3 occupancy bit sets of the raw clouds, uint32 [P][2][1024], voxel (x*32 + y)*32 + z = bit (v & 31) of word v >> 5
 *   TOTAL       = pcd_pair_metrics_workspace_bytes(pairs, na_max, nb_max)
 * ALPHA .. ERR are written only by a call with with_sinkhorn.  Host arithmetic only: no device is touched. */
enum { PCD_PAIR_WS_AN = 0, PCD_PAIR_WS_BN, PCD_PAIR_WS_MINS, PCD_PAIR_WS_ALPHA, PCD_PAIR_WS_BETA, PCD_PAIR_WS_ROWC,
       PCD_PAIR_WS_CMAX, PCD_PAIR_WS_ERR, PCD_PAIR_WS_BITS, PCD_PAIR_WS_TOTAL, PCD_PAIR_WS_FIELDS };
int pcd_pair_metrics_workspace_layout(int pairs, int na_max, int nb_max, size_t* offsets);

/* ---- surface evaluation of a batch of independent cloud pairs (csrc/surface_metrics.hip; DESIGN.md "Surface metrics") ----
 * The packing of pcd_pair_metrics: pair p = q[p][0..nq[p]) vs t[p][0..nt[p]) inside padded fp32 arrays [P][nq_max][3] / [P][nt_max][3], counts
 * device int32 [P] (a count below 0 counts as 0, one above the padded size as that size); rows at or past a count are never read.  All distance
 * and dot-product arithmetic is fp32 without contraction, so every stage below is an exact statement.
 * Nearest neighbour.  For every query i < nq[p]: d2[p][i] = min_j ((dx dx + dy dy) + dz dz) over the targets j < nt[p] whose value is finite,
 * from direct differences, and index[p][i] = the LOWEST j that attains it.  A query with no finite distance to any target -- a query or every
 * target with a coordinate that is not finite, or no targets -- gets d2 = NaN, index = -1, as does every row at or past the count; a target that
 * is not finite is never anyone's neighbour.  d2 fp32 [P][nq_max], index int32 [P][nq_max].  The target range is split over the grid; the
 * partial results meet in a 64-bit unsigned atomic min on (bits of d2) << 32 | j, so the result is bitwise repeatable and independent of the
 * split count and of the rest of the batch.  workspace: pcd_nearest_workspace_bytes() bytes (host arithmetic, 0 for arguments the call refuses),
 * any contents.  One enqueue, no host synchronisation.  PCD_ERR_ARG (before any device work) for a null pointer, pairs <= 0 or > 65535, a
 * padded size <= 0, or a workspace that is too small. */
size_t pcd_nearest_workspace_bytes(int pairs, int nq_max, int nt_max);
int pcd_nearest_neighbors(const float* q, const int* nq, int nq_max, const float* t, const int* nt, int nt_max, int pairs, float* d2,
                          int32_t* index, void* workspace, size_t workspace_bytes, void* stream);
/* Rows.  Both directions of all pairs (a queries b, b queries a) through the nearest-neighbour kernel in one launch, then one workgroup per
 * pair: rows fp32 [P][PCD_SURF_ROW_BASE + 3 n_thresholds].  With d = sqrtf(d2) per query:
 *   ACC, COMP          the mean of d over a, over b            ACC2, COMP2   the means of d2
 *   CHAMFER_L1         (ACC + COMP) / 2                        CHAMFER_L2    ACC2 + COMP2
 *   HAUSDORFF          sqrtf of the largest d2 of both directions
 *   NC_A, NC_B         the mean over a (over b) of |n . n'[index]| = fabsf((x x' + y y') + z z'), n the query's normal and n' the normal of its
 *                      nearest neighbour; NC = (NC_A + NC_B) / 2.  The absolute value makes it blind to a flipped winding, on purpose.  NaN
 *                      when normals_a or normals_b (fp32, packed as the clouds) is null.
 *   BASE + 3k ..       threshold tau_k: PRECISION = |{i in a: d2 <= tau_k tau_k}| / na (one fp32 product, an integer count, one fp32 division),
 *                      RECALL the same over b, FSCORE = (2 P R) / (P + R), 0 when P + R = 0.
 * The means are accumulated in double in a fixed order (per-thread strided partials, a butterfly over each wave, the four waves in order) and
 * rounded to fp32 once; the derived columns are fp32 operations on those.  A pair with a count of 0, or with a point that has no finite
 * distance to the other cloud (any coordinate inside the counts that is not finite, on either side), gets an all-NaN row; the other pairs are
 * not affected.  thresholds: HOST fp32 [n_thresholds], 0 <= n_thresholds <= PCD_SURF_MAX_THRESHOLDS.  Optional outputs (null: not written):
 * d2_a / index_a [P][na_max] and d2_b / index_b [P][nb_max], the nearest-neighbour results of the two directions as pcd_nearest_neighbors
 * defines them.  workspace: pcd_surface_metrics_workspace_bytes() bytes, any contents.  PCD_ERR_ARG (before any device work) for a null a, na,
 * b, nb, rows or workspace, pairs <= 0 or 2 pairs > 65535, a padded size <= 0, n_thresholds outside 0 .. 8 (or > 0 with null thresholds), a
 * threshold that is negative or not finite, or a workspace that is too small. */
#define PCD_SURF_MAX_THRESHOLDS 8
enum { PCD_SURF_ROW_ACC = 0, PCD_SURF_ROW_COMP, PCD_SURF_ROW_CHAMFER_L1, PCD_SURF_ROW_ACC2, PCD_SURF_ROW_COMP2, PCD_SURF_ROW_CHAMFER_L2,
       PCD_SURF_ROW_HAUSDORFF, PCD_SURF_ROW_NC_A, PCD_SURF_ROW_NC_B, PCD_SURF_ROW_NC, PCD_SURF_ROW_BASE };
size_t pcd_surface_metrics_workspace_bytes(int pairs, int na_max, int nb_max);
int pcd_surface_metrics(const float* a, const float* normals_a, const int* na, int na_max, const float* b, const float* normals_b,
                        const int* nb, int nb_max, int pairs, const float* thresholds, int n_thresholds, float* rows, float* d2_a,
                        int32_t* index_a, float* d2_b, int32_t* index_b, void* workspace, size_t workspace_bytes, void* stream);
/* out[p] = |A and B| / |A or B| of two fp32 grids [P][voxels] with occupancy value > threshold: integer counts, one fp32 division, NaN for an
 * empty union.  PCD_ERR_ARG for a null pointer, pairs <= 0, voxels <= 0 or a threshold that is not finite. */
int pcd_voxel_iou(const float* a, const float* b, int pairs, int voxels, float threshold, float* out, void* stream);

/* ---- local geometry of a batch of independent clouds (csrc/cloud_geometry.hip; DESIGN.md "Cloud geometry") ----
 * The packing of the surface evaluation above: cloud p = points[p][0..counts[p]) inside a padded fp32 array [P][n_max][3], counts device int32 [P]
 * (below 0 counts as 0, above the padded size as that size); rows at or past a count are never read as data.  Every call is one enqueue with no
 * host synchronisation, bitwise repeatable, and a cloud's result does not depend on the rest of the batch.  PCD_ERR_ARG (before any device work)
 * for a null required pointer, clouds <= 0 or > 65535, a padded size <= 0, k outside 1 .. PCD_KNN_MAX_K, or what an entry point names below.
 * k nearest.  For every query i < nq[p] the k nearest targets j < nt[p], sorted: d2 fp32 [P][nq_max][k], index int32 [P][nq_max][k].  d2 =
 * (dx dx + dy dy) + dz dz in fp32 from direct differences without contraction (the arithmetic of pcd_nearest_neighbors); the candidates are
 * ordered by the key (bits of d2) << 32 | j, so slot 0 is the nearest and equal distances go to the lower j.  A target whose d2 is not finite
 * is nobody's neighbour.  With exclude_self the target j == i (the query's own row) is skipped and nothing else is -- the caller passes the
 * same array as q and t; a duplicate of the point at another index is a neighbour at distance 0.  A query with fewer than k candidates has
 * (NaN, -1) in the trailing slots; a query with a coordinate that is not finite, and every row at or past nq[p], has (NaN, -1) in every slot.
 * Slot s does not depend on k. */
#define PCD_KNN_MAX_K 32
int pcd_knn(const float* q, const int* nq, int nq_max, const float* t, const int* nt, int nt_max, int clouds, int k, int exclude_self,
            float* d2, int32_t* index, void* stream);
/* Normals by principal component analysis of the neighbour lists index [P][n_max][k] (pcd_knn with exclude_self).  The neighbourhood of point i
 * is the point itself and its neighbours 0 <= index < counts[p] (other entries are skipped).  With fewer than 3 members: normal (0, 0, 0),
 * curvature NaN.  Otherwise the covariance about the neighbourhood's own mean, with eigenvalues l0 <= l1 <= l2: the normal is the unit
 * eigenvector of l0 and the curvature l0 / (l0 + l1 + l2) (NaN for a trace of 0).  All of it is computed in double from the differences to
 * point i and rounded to fp32 once, so |n| = 1 to an fp32 rounding; where l0 = l1 the direction is one of the plane's, still of unit length.
 * mode: PCD_NORMALS_UNORIENTED (the sign is unspecified but repeatable), PCD_NORMALS_OUTWARD (n . (p - c) >= 0 with c the mean, accumulated
 * in double, of the cloud's rows below the count whose coordinates are finite), PCD_NORMALS_TOWARD_VIEW (n . (v - p) >= 0 with v =
 * viewpoints[p], fp32 [P][3]).  normals fp32 [P][n_max][3]; curvature fp32 [P][n_max] or null.  Rows at or past the count, and a neighbourhood
 * with a coordinate that is not finite: zero normal, NaN curvature.  workspace: pcd_cloud_normals_workspace_bytes() bytes, any contents, read
 * and written only under PCD_NORMALS_OUTWARD (null otherwise is fine).  PCD_ERR_ARG also for an unknown mode, PCD_NORMALS_TOWARD_VIEW with
 * null viewpoints, PCD_NORMALS_OUTWARD with a workspace that is null or too small. */
enum { PCD_NORMALS_UNORIENTED = 0, PCD_NORMALS_OUTWARD = 1, PCD_NORMALS_TOWARD_VIEW = 2 };
size_t pcd_cloud_normals_workspace_bytes(int clouds);
int pcd_cloud_normals(const float* points, const int* counts, int n_max, int clouds, const int32_t* index, int k, int mode,
                      const float* viewpoints, float* normals, float* curvature, void* workspace, size_t workspace_bytes, void* stream);
/* Outlier mask from the neighbour distances d2 [P][n_max][k] of pcd_knn (a NaN slot is not valid).  dbar_i = the mean over the valid slots of
 * sqrtf(d2): correctly rounded fp32 roots, summed in slot order and divided in double.  PCD_OUTLIER_STATISTICAL: a point without a valid slot
 * is dropped and takes no part in the statistics; mu and sigma (the population standard deviation, two passes) over the points that have a
 * dbar, in double in a fixed order; the point is kept iff dbar_i <= mu + std_ratio sigma, compared in double.  PCD_OUTLIER_RADIUS: the point is
 * kept iff at least min_neighbors slots have d2 <= radius * radius, one fp32 product.  mask uint8 [P][n_max], 1 = keep, 0 at and past the count;
 * mean_distance fp32 [P][n_max] or null: dbar_i rounded to fp32, NaN without a valid slot and at and past the count.  PCD_ERR_ARG also for an
 * unknown method, a std_ratio that is not finite, a radius that is negative or not finite, min_neighbors outside 1 .. k. */
enum { PCD_OUTLIER_STATISTICAL = 0, PCD_OUTLIER_RADIUS = 1 };
int pcd_cloud_outlier_mask(const float* d2, const int* counts, int n_max, int clouds, int k, int method, double std_ratio, float radius,
                           int min_neighbors, uint8_t* mask, float* mean_distance, void* stream);
/* Stable compaction: the rows i < counts[p] with mask[p][i] != 0 move, in their order, to the front of points_out[p] (and those of the
 * optional second array attr [P][n_max][3], normals for instance, to attr_out), the rows behind them are set to zero and counts_out[p] is their
 * number.  Nothing is read back.  PCD_ERR_ARG also for attr without attr_out (or the reverse) and for an output that is its input. */
int pcd_cloud_compact(const float* points, const float* attr, const uint8_t* mask, const int* counts, int n_max, int clouds,
                      float* points_out, float* attr_out, int* counts_out, void* stream);

/* ---- closed meshes from clouds by grid closing (csrc/cloud_mesh.hip; definition in DESIGN.md "Cloud to mesh") ----
 * The clouds are packed as above.  The grid has R nodes per axis, 8 <= R <= 64; node i of an axis sits at lo + (float)i * h in fp32, the
 * product rounded, then the sum; h = (hi - lo) / (R - 1) is computed by the caller in double and passed as fp32.  Grids are indexed [z][y][x].
 * A row (z, y) of node bits is one uint64 word, bit x = node x, bits at and past R are 0 on output and ignored on input.  Every call is one
 * enqueue (pcd_grid_depth_field: two) with no host synchronisation, bitwise repeatable, a cloud's result independent of the rest of the batch.
 * PCD_ERR_ARG (before any device work) for a null required pointer, clouds <= 0 or > 65535, R outside 8 .. 64, lo or h that is not finite,
 * h <= 0, inset outside [-1, 1], or what an entry point names below.
 *
 * Radius.  With d2 [P][n_max][k] (pcd_knn with exclude_self; the issue's k = 8) and radii_in null: s_p = the mean, over the rows below the count
 * whose slot k - 1 is valid, of sqrtf(d2[.][k - 1]) (correctly rounded fp32 roots, summed in double, rounded to fp32 once), r_p = radius_scale *
 * s_p, 0 without such a row.  With radii_in fp32 [P] and d2 null: r_p = radii_in[p].  Either way radii[p] = max(r_p, (2 - inset) * h), the
 * clamp in fp32 as written, which a NaN r_p takes too.  PCD_ERR_ARG also for both or neither of d2 and radii_in, and with d2 for null counts,
 * n_max <= 0, k outside 1 .. PCD_KNN_MAX_K, a radius_scale that is not finite or <= 0. */
int pcd_cloud_spacing(const float* d2, const int* counts, int n_max, int clouds, int k, const float* radii_in, float radius_scale, float h,
                      float inset, float* radii, void* stream);
/* Shell and outside in one launch, one workgroup per cloud with both masks in LDS.  Node (z, y, x) is shell iff some row i < counts[p] with three
 * finite coordinates has (dx dx + dy dy) + dz dz <= radii[p] * radii[p], the differences from the node coordinates above, all fp32 without
 * contraction.  Free = not shell; outside = the free nodes 6-connected through free nodes to the layer of free nodes that is thought round the
 * grid.  shell, outside uint64 [P][R][R]; info int32 [P][3] = (shell nodes, enclosed nodes = free and not outside, shell nodes on the six faces
 * of the grid); sweeps int32 [P] or null: the sweeps the fill took, -1 had it passed R^3 (it cannot: every sweep but the last gains a node).
 * The radii must be finite; the cost grows with n (r / h)^2.  PCD_ERR_ARG also for n_max <= 0. */
int pcd_cloud_shell_fill(const float* points, const int* counts, int n_max, int clouds, int resolution, float lo, float h, const float* radii,
                         uint64_t* shell, uint64_t* outside, int32_t* info, int32_t* sweeps, void* stream);
/* The fill alone, on the caller's shell words [P][R][R]; outputs as above.  PCD_ERR_ARG also for outside == shell. */
int pcd_grid_fill_outside(const uint64_t* shell, int clouds, int resolution, uint64_t* outside, int32_t* info, int32_t* sweeps, void* stream);
/* d2 int32 [P][R][R][R] or null: the squared Euclidean distance in pitches from every node to the nearest outside node, the layer round the grid
 * counting as outside (the exact integer transform, 0 on outside nodes).  v fp32 [P][R][R][R]: 0 where d2 = 0, elsewhere
 * 1.0f + ((sqrtf((float)d2) * h - radii[p]) - inset * h) in fp32 in that order without contraction; the closed solid is v > 1.  v holds
 * intermediate integers between the two launches.  PCD_ERR_ARG also for d2 == v. */
int pcd_grid_depth_field(const uint64_t* outside, int clouds, int resolution, float h, const float* radii, float inset, int32_t* d2, float* v,
                         void* stream);
/* out[p][i] = scale * vertices[p][i] + offset per component (fp32, product then sum) for i < vertex_counts[p], vertices and out fp32
 * [P][v_max][3] (out may be vertices); rows at and past the count are not written.  With index int32 [P][v_max][k] (pcd_knn of the mapped vertices
 * against the clouds) the mapped vertex v is then projected: over its neighbours 0 <= index < counts[p], their mean c and their covariance about
 * c, n the unit eigenvector of the least eigenvalue, out = v - ((v - c) . n) n, all in double from the differences to v, rounded to fp32 once;
 * with fewer than 3 neighbours, or a result that is not finite, out = v.  PCD_ERR_ARG also for v_max <= 0, a scale or offset that is not
 * finite, and with index for null points or counts, n_max <= 0, k outside 1 .. PCD_KNN_MAX_K. */
int pcd_project_to_cloud(const float* vertices, const int* vertex_counts, int v_max, const float* points, const int* counts, int n_max,
                         int clouds, const int32_t* index, int k, float scale, float offset, float* out, void* stream);

/* ------------------------------------------------ training step of the point denoiser
 * diffusion.py:70-86,170-186 (add_noise -> model in train() mode -> F.l1_loss -> AdamW, diffusion.py:60).
 * The dense products (forward, backward-data, backward-weight) are pcd_gemm_f16* calls; these entry points
 * are the BatchNorm1d-with-batch-statistics forward/backward (networks.py:31-48), the max-pool with its
 * argmax (networks.py:807), the K=3 / C=3 edge layers, reductions, transposes, loss and optimizer.
 * Activations / activation gradients fp16 [M][C]; statistics, parameter gradients, optimizer state fp32.
 * Gradients carry the caller's loss scale; pcd_adamw_step divides it out.
 * Column widths: pcd_colsum_f16, pcd_bn_apply_f16, pcd_bn_backward_f16 and pcd_vec3_outer (its k) serve any c > 0.  With
 * c % 8 == 0 (16-byte aligned base pointers: every row then starts 16-byte aligned) they read and write 8 columns in
 * 16-byte accesses; with any other c, c = 1 included, every element is accessed on its own.  pcd_bn_batch_stats
 * requires c % 8 == 0 and rejects other widths with PCD_ERR_ARG. */
/* out[g][c] = sum over the rows_per_group rows of group g of x[row][c]   (bias gradients, per-shape sums) */
int pcd_colsum_f16(const void* x, int64_t rows_per_group, int groups, int c, float* out, void* stream);
/* BatchNorm1d training statistics over the M rows of the fp32 conv output z [M][c] (c % 8 == 0): mean[c], biased
 * var[c] (one pass, sums shifted by row 0 so that E[d^2] - E[d]^2 does not cancel); if running_* are given they are updated as torch does (momentum, UNBIASED variance).
 * scratch: fp32 [2*c]. */
int pcd_bn_batch_stats(const float* z, int64_t m, int c, float momentum, float* mean, float* var,
                       float* running_mean, float* running_var, float* scratch, void* stream);
/* a = act(gamma * (z - mean) / sqrt(var + eps) + beta) -> fp16, act = ReLU if relu; z fp32 */
int pcd_bn_apply_f16(const float* z, int64_t m, int c, const float* mean, const float* var, const float* gamma,
                     const float* beta, float eps, int relu, void* out, void* stream);
/* backward of pcd_bn_apply_f16 with batch statistics: da -> dz, dgamma[c], dbeta[c] */
int pcd_bn_backward_f16(const void* da, const float* z, int64_t m, int c, const float* mean, const float* var,
                        const float* gamma, const float* beta, float eps, int relu, float* dgamma, float* dbeta,
                        void* dz, void* stream);
/* dst[c][r] = src[r][c]  (operands of the backward-weight product dW = dz^T a) */
int pcd_transpose_f16(const void* src, int64_t rows, int cols, void* dst, void* stream);
/* torch.max(x, 2) of networks.py:807 on a [B*N][C]: per shape and channel the max and the FIRST index attaining it */
int pcd_colmax_argmax_f16(const void* a, int batch, int n_points, int c, float* mx, int* arg, void* stream);
/* its backward: da = 0 except da[b*N + arg[b][c]][c] = dg[b][c] */
int pcd_maxpool_backward_f16(const float* dg, const int* arg, int batch, int n_points, int c, void* da, void* stream);
/* enc1.conv1 before its BatchNorm: z[m][c] = sum_j x[m][j] w_xyz[c][j] + tbias[m / n_points][c]; x fp32 [M][3], z fp32 */
int pcd_enc1_linear(const float* x, int64_t m, int n_points, const float* w_xyz, int c1, const float* tbias,
                    float* out, void* stream);
/* out[j][k] = sum_m vec[m][j] * mat[m][k], j < 3 (dW of the 64->3 head and of enc1's xyz columns); vsum[j] = sum_m vec[m][j] or NULL */
int pcd_vec3_outer(const void* mat, const float* vec, int64_t m, int k, float* out, float* vsum, void* stream);
/* out[m][k] = sum_j vec[m][j] * w[j][k]  (backward-data of the 64->3 head) */
int pcd_vec3_expand_f16(const float* vec, const float* w, int64_t m, int k, void* out, void* stream);
/* F.l1_loss(noise, pred) of diffusion.py:182: loss_sum[0] = sum |pred - target| (divide by n on the host),
 * dpred = grad_scale * sign(pred - target) / n */
int pcd_l1_loss(const float* pred, const float* target, int64_t n, float grad_scale, float* loss_sum, float* dpred,
                void* stream);
/* small fp32 product C[m][n] (+)= op(A)[m][k] op(B)[k][n] + bias[n]: time_mlp and the per-shape bias paths */
int pcd_matmul_f32(const float* a, int64_t lda, int trans_a, const float* b, int64_t ldb, int trans_b, int m, int n,
                   int k, const float* bias, int accumulate, float* c, int64_t ldc, void* stream);
int pcd_silu_f32(const float* x, int64_t n, float* y, void* stream);
int pcd_silu_backward_f32(const float* x, const float* dy, int64_t n, float* dx, void* stream);
/* latent denoiser training (networks.py:977-1049: Linear + GroupNorm(8) + ReLU on (B, C) rows; all fp32, B = batch):
 * GroupNorm forward keeping (mean, rstd) [rows][groups], and its backward (dx, dgamma, dbeta), ReLU folded in if relu */
int pcd_groupnorm_f32(const float* x, int rows, int c, int groups, const float* gamma, const float* beta, float eps,
                      int relu, float* y, float* mean, float* rstd, void* stream);
int pcd_groupnorm_backward_f32(const float* dy, const float* x, int rows, int c, int groups, const float* gamma,
                               const float* beta, const float* mean, const float* rstd, int relu, float* dx,
                               float* dgamma, float* dbeta, void* stream);
/* y = x * mask * scale: nn.Dropout forward with a given keep mask (scale = 1/(1-p)) and, applied to dy, its backward */
int pcd_mask_scale_f32(const float* x, const float* mask, float scale, int64_t n, float* y, void* stream);
int pcd_relu_f32(const float* x, int64_t n, float* y, void* stream);
int pcd_relu_backward_f32(const float* x, const float* dy, int64_t n, float* dx, void* stream);
/* voxel VAE training (networks.py:2225-2264, 471-504): a Conv3d / ConvTranspose3d layer as "gather rows, then the GEMM".
 * Channels-last fp16 rows [b*D*H*W][C]; cubic kernel k, stride, pad; transposed = 1 for ConvTranspose3d indexing.
 * col[r][t*cin + c] = x[source of output r at tap t][c] or 0, row length kp >= k^3*cin (extra columns zeroed);
 * pcd_col2im_f16 is its adjoint as a gather: dx[i][c] = sum_t dcol[output that reads i at tap t][t*cin + c]. */
int pcd_im2col_f16(const void* x, int batch, int cin, int di, int hi, int wi, int d_o, int ho, int wo, int k, int stride,
                   int pad, int transposed, int kp, void* col, void* stream);
int pcd_col2im_f16(const void* dcol, int batch, int cin, int di, int hi, int wi, int d_o, int ho, int wo, int k, int stride,
                   int pad, int transposed, int kp, void* dx, void* stream);
/* out[r][c] = act(x[r][c] + bias[c]): a ConvTranspose3d is run as product-then-col2im (the adjoint of a Conv3d), its
 * bias and ReLU applied afterwards */
int pcd_bias_act_f16(const void* x, const float* bias, int64_t rows, int c, int relu, void* out, void* stream);
/* out = a + b, with ReLU if relu (ResidualBlock3D tail); d = dout * [out > 0] */
int pcd_add_relu_f16(const void* a, const void* b, int64_t n, int relu, void* out, void* stream);
int pcd_relu_mask_f16(const void* dout, const void* out, int64_t n, void* d, void* stream);
/* recon = sigmoid(logit[i*ld]); loss_sum[0] = sum BCE(recon, target) with torch's -100 log clamp (networks.py:2387);
 * dlogit[i*ld] = grad_scale * (recon - target) / n  (BCE and Sigmoid backward fused) */
int pcd_sigmoid_bce(const void* logit, int64_t ld, const float* target, int64_t n, float grad_scale, float* loss_sum,
                    float* recon, void* dlogit, void* stream);
/* backward of z = mu + eps * exp(logvar / 2) and of kl_scale * KL (networks.py:2323-2325, 2389-2396) over n = B * latent
 * elements: dmu, dlogvar; kl_sum[0] = sum(1 + logvar - mu^2 - exp(logvar)) (KL = -0.5 * kl_sum / n) */
int pcd_vae_latent_backward(const float* mu, const float* logvar, const float* eps, const float* dz, int64_t n,
                            float kl_scale, float* dmu, float* dlogvar, float* kl_sum, void* stream);
/* torch.optim.AdamW step on one flat fp32 buffer (diffusion.py:60: lr, weight_decay 1e-5); grads are divided by grad_scale */
int pcd_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* The same step (params, exp_avg, exp_avg_sq come out bitwise equal) and, in the same launch, the exponential moving
 * average of the weights: ema[i] = ema_decay * ema[i] + (1 - ema_decay) * params_new[i]; ema_decay in [0, 1) */
int pcd_adamw_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                       float ema_decay, void* stream);

/* ------------------------------------------------ gradient guard: norm, non-finite scan, clipping, skipped steps, accumulation
 * None of these synchronises the stream or copies to the host; what the guard decides stays on the device, in a state
 * block of 16 32-bit words (64 bytes, 4-byte aligned, zero-filled by the caller before first use) that only
 * these two entry points write and read:
 *   word 0  float  norm       norm of the unscaled gradient seen by the last pcd_grad_norm_f32
 *   word 1  int    apply      1: the step is taken; 0: a gradient element was non-finite, the step is dropped
 *   word 2  float  coef       clip coefficient min(1, max_norm / (norm + 1e-6)); exactly 1.0f without clipping, 0 when dropped
 *   word 3  float  inv_scale  (1.f / grad_scale) * coef: what the guarded AdamW multiplies the gradients by
 *   word 4  float  bc1        AdamW's bias corrections 1 - beta^t for this step (see below)
 *   word 5  float  bc2
 *   word 6  int    applied    running count of steps taken
 *   word 7  int    skipped    running count of steps dropped
 *   word 8  int    clipped    running count of steps taken with coef < 1
 *   words 9-15     reserved (left as they are)
 * The caller may preset the counters (resuming a run); it keeps applied + skipped equal to `step` - 1 before a call. */
/* One pass over grads[n] (16-byte loads when the pointer is 16-byte aligned, else one element per lane; launch geometry
 * fixed by n): the squares are summed in double, block partials are added in index order by one block (no atomics: the
 * result is bitwise repeatable), an element whose exponent bits are all ones makes the buffer non-finite.  The same
 * block then writes the state block: norm = sqrt(sum) / grad_scale formed in double and rounded to fp32 once; apply;
 * coef (max_norm <= 0: no clipping); inv_scale; the counters.  A dropped step does not advance AdamW's step: while
 * skipped == 0 the bias corrections are the host's 1.f - powf(beta, (float)step), exactly those of pcd_adamw_step for
 * that step, afterwards they are recomputed on the device for t = step - skipped. */
int pcd_grad_norm_f32(const float* grads, int64_t n, float grad_scale, float max_norm, int step, float beta1, float beta2,
                      void* state, void* stream);
/* pcd_adamw_step / pcd_adamw_ema_step (ema may be NULL; the same element update, bitwise) taking inv_scale, bc1, bc2 and
 * the apply flag from the state block: with apply == 0 nothing is read or written besides the block */
int pcd_adamw_guarded_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                           const void* state, void* stream);
/* acc[i] = grads[i] if first, else acc[i] + grads[i]  (gradient accumulation over micro-batches) */
int pcd_grad_accumulate_f32(float* acc, const float* grads, int64_t n, int first, void* stream);

/* ------------------------------------------------ class embedding of the class-conditional point denoiser
 * temb[b][:] += table[labels[b]][:] for temb [batch][dim], table [rows][dim], device int32 labels[batch]; a label outside
 * [0, rows) adds nothing */
int pcd_embed_add_rows(float* temb, const float* table, const int* labels, int batch, int dim, int rows, void* stream);
/* its backward: dtable[c][:] = the sum of dtemb[b][:] over the shapes with labels[b] == c, added in ascending b in fp32, one
 * lane per (c, column), no atomics (bitwise repeatable); a row without shapes is written as zero */
int pcd_embed_rows_backward(const float* dtemb, const int* labels, int batch, int dim, int rows, float* dtable, void* stream);

/* ------------------------------------------------ device-resident voxel dataset (csrc/dataset.hip)
 * grids: [n_grids][1024] 32-bit words, one 32^3 occupancy grid each: word z * 32 + y, bit x.  Ascending (word, bit) is
 * numpy.where's row-major order of grid[z][y][x], the scan order of PointCloudDataset.voxel_to_point_cloud, and a point is the
 * integer triple (z, y, x) in that column order.  index[batch]: device int32 grid numbers; one outside [0, n_grids) reads
 * nothing, gives zero rows and counts[b] = -1.
 *
 * Randomness is Philox4x32-10 as in pcd_randn: counter words {lo(ctr), hi(ctr), 0, 0}, key {lo(seed), hi(seed)}.  Batch slot b
 * owns the PCD_VOXEL_CTR_SPAN counters from offset + b * PCD_VOXEL_CTR_SPAN; inside its span (counter numbers relative to it)
 *   [PCD_VOXEL_CTR_KEY,    + 8192)    subset keys: the key of point i (its ordinal in scan order) is word i & 3 of counter i >> 2
 *    PCD_VOXEL_CTR_ANGLE               rotation: angle = 2 pi u, u = ((word 0 >> 8) + 0.5) / 2^24
 *   [PCD_VOXEL_CTR_JITTER, + 32768)   jitter: counter i gives point i its normals, pcd_randn's Box-Muller values 0, 1, 2 of the
 *                                     counter for columns 0, 1, 2 (value 3 is not used)
 *   [PCD_VOXEL_CTR_DRAW,   SPAN)      draws with replacement: draw j is word j & 3 of counter j >> 2
 * so slot b's rows depend on (grid, seed, offset, b, num_points, flags) only, not on the rest of the batch. */
#define PCD_VOXEL_NORMALIZE 1
#define PCD_VOXEL_ROTATE 2
#define PCD_VOXEL_JITTER 4
#define PCD_VOXEL_CTR_KEY 0ull
#define PCD_VOXEL_CTR_ANGLE 8192ull
#define PCD_VOXEL_CTR_JITTER 16384ull
#define PCD_VOXEL_CTR_DRAW 65536ull
#define PCD_VOXEL_CTR_SPAN (1ull << 24)
#define PCD_VOXEL_MAX_POINTS (1 << 24)          /* 4 draws per counter: far inside the draw range */
/* out[batch][num_points][3], counts[batch] = M, the occupied voxels of each slot's grid; one workgroup per slot, no host
 * synchronisation.  PointCloudDataset._load's chain for voxel files and point-cloud output:
 *   rotate     centre on the centroid and scale to unit radius (as below), then right-multiply by the rotation about column 1
 *   jitter     add clip(sigma * normal, -clip, clip) to every coordinate of all M points
 *   normalize  p = (p - mean) / radius, radius = max |p - mean|.  Without rotate and jitter the column sums are integers
 *              < 2^24 (exact): mean = float(sum) / float(M), radius = sqrt(max((dz dz + dy dy) + dx dx)), all in fp32 without
 *              contraction, division and root correctly rounded: bit-exact against the same numpy operations.  After an
 *              augmentation the sums are fp32, added in a fixed order (bitwise repeatable).
 *   resample   M = num_points: every point in scan order.  M > num_points: the num_points smallest (key, i) pairs, written in
 *              ascending i (a uniform subset without replacement, in scan order; the cut is found by a radix select over the
 *              keys, which are regenerated in every pass and never stored).  M < num_points: every point in scan order, then
 *              num_points - M draws in draw order, draw -> point (word * M) >> 32.
 * M = 0 gives zero rows.  A cloud of radius 0 under normalize or rotate (M = 1) gives NaN rows, 0 / 0 as in the host's
 * normalize_point_cloud: callers keep such grids out of the table (DeviceVoxelDataModule refuses them).
 * num_points <= PCD_VOXEL_MAX_POINTS. */
int pcd_voxel_batch_clouds(const uint32_t* grids, int n_grids, const int* index, int batch, int num_points, uint64_t seed,
                           uint64_t offset, int flags, float sigma, float clip, float* out, int* counts, void* stream);
/* out[batch][1][32][32][32] = 0.f / 1.f, [z][y][x]: the indexed grids unpacked (an index outside the table gives zeros) */
int pcd_voxel_batch_grids(const uint32_t* grids, int n_grids, const int* index, int batch, float* out, void* stream);

/* ------------------------------------------------ device-resident mesh dataset (csrc/mesh_data.hip; DESIGN.md "Mesh dataset")
 * The table: n_meshes meshes in the packing of pcd_mesh_sample_points -- vertices fp32 [sum V][3], faces int32 [sum F][3] local to
 * the mesh, offsets int64 [n_meshes + 1][2] -- and area_sums fp32 [sum F], the per-mesh inclusive running sums of the triangle
 * areas.  pcd_mesh_area_sums writes them: it IS launch 1 of pcd_mesh_sample_points (same kernel, same tree, a non-finite area
 * counts as 0), so area_sums is bitwise that call's workspace.  Once per table.  PCD_ERR_ARG for a null pointer or n_meshes <= 0. */
int pcd_mesh_area_sums(const float* vertices, const int32_t* faces, const int64_t* offsets, int n_meshes, float* area_sums, void* stream);
/* out fp32 [batch][num_points][3]: slot b is a cloud of num_points points drawn uniformly by area from mesh index[b] (device int32),
 * then sent through the chain of pcd_voxel_batch_clouds.  normals (optional, fp32 [batch][num_points][3]): the unit normal of each
 * point's face; face_index (optional, int32 [batch][num_points]): that face, local to the mesh.  One workgroup per slot, one launch,
 * no workspace, no host synchronisation, no float atomics: bitwise repeatable.
 *
 * Randomness is Philox4x32-10 as in pcd_randn: counter words {lo(ctr), hi(ctr), 0, 0}, key {lo(seed), hi(seed)}.  Batch slot b owns
 * the PCD_MESH_CTR_SPAN counters from offset + b * PCD_MESH_CTR_SPAN; inside its span (counter numbers relative to it)
 *   [PCD_MESH_CTR_POINT,  + num_points)  counter i gives point i its u0, u1, u2 as pcd_mesh_sample_points derives them:
 *                                        u_k = (word k >> 8) / 2^24 (word 3 is not used)
 *    PCD_MESH_CTR_ANGLE                  rotation: angle = 2 pi u, u = ((word 0 >> 8) + 0.5) / 2^24 (PCD_VOXEL_CTR_ANGLE's formula)
 *   [PCD_MESH_CTR_JITTER, + num_points)  jitter: counter i gives point i its normals, pcd_randn's Box-Muller values 0, 1, 2 of the
 *                                        counter for columns 0, 1, 2 (value 3 is not used), as PCD_VOXEL_CTR_JITTER does
 * The ranges are 2^24 counters apart and num_points <= PCD_MESH_MAX_POINTS = 2^24, so they cannot meet.  Slot b's rows depend on
 * (mesh, seed, offset, b, num_points, flags) only, not on the rest of the batch.
 *
 * Draw.  Triangle f is the first of the mesh whose running sum exceeds u0 * total (the last one at most), total the mesh's last
 * running sum; the point is (1 - s) A + s (1 - u2) B + s u2 C with s = sqrt(u1), evaluated per coordinate as
 * ((1 - s) a + (s (1 - u2)) b) + (s u2) c in fp32 without contraction.  With flags = 0 slot b is bitwise pcd_mesh_sample_points on
 * mesh index[b] alone with philox_offset = offset + b * PCD_MESH_CTR_SPAN + PCD_MESH_CTR_POINT: points, normals and face_index.
 *
 * Chain.  flags are PCD_VOXEL_NORMALIZE, PCD_VOXEL_ROTATE, PCD_VOXEL_JITTER with the meaning and order of pcd_voxel_batch_clouds:
 *   rotate     centre on the centroid and scale to unit radius (as below), then right-multiply by the rotation about column 1,
 *              [[c, 0, s], [0, 1, 0], [-s, 0, c]]: p0' = p0 c - p2 s, p2' = p0 s + p2 c
 *   jitter     add clip(sigma * normal, -clip, clip) to every coordinate
 *   normalize  p = (p - mean) / radius, mean = sum / float(num_points), radius = sqrt(max((d0 d0 + d1 d1) + d2 d2)) over the points,
 *              d = p - mean
 * Every cloud has exactly num_points points: there is no resample stage.  All of it is fp32 without contraction, division and root
 * correctly rounded.  The column sums of a centroid are added in this fixed order: lane t of the 1024 adds the points t, t + 1024,
 * t + 2048, ... in ascending order to a partial that starts at 0; inside each wave (lanes 64 w .. 64 w + 63) the partials are
 * combined by the butterfly x[l] = x[l] + x[l ^ o] for o = 32, 16, 8, 4, 2, 1; the 16 wave sums are then added in ascending w,
 * starting from wave 0's.  The radius is a max and does not depend on the order.  tests/mesh_data_statement.py reproduces the sums:
 * given the device's sine, cosine and normals the rows are bit-exact against the same numpy operations.  normals are rotated with
 * the points; jitter and normalisation do not change them.
 *
 * An index outside [0, n_meshes), a mesh without vertices or faces, or one whose total area is not above 0 gives zero rows, zero
 * normals and face_index -1.  A cloud of radius 0 under normalize or rotate (every point the same) gives NaN rows, 0 / 0 as in
 * pcd_voxel_batch_clouds.  PCD_ERR_ARG (before any device work) for a null vertices, faces, offsets, area_sums, index or out,
 * n_meshes <= 0, batch <= 0, num_points <= 0 or > PCD_MESH_MAX_POINTS, an unknown flag, or a non-finite sigma or clip. */
#define PCD_MESH_CTR_POINT 0ull
#define PCD_MESH_CTR_ANGLE (1ull << 24)
#define PCD_MESH_CTR_JITTER (1ull << 25)
#define PCD_MESH_CTR_SPAN (1ull << 26)
#define PCD_MESH_MAX_POINTS (1 << 24)
int pcd_mesh_batch_clouds(const float* vertices, const int32_t* faces, const int64_t* offsets, int n_meshes, const float* area_sums,
                          const int* index, int batch, int num_points, uint64_t seed, uint64_t offset, int flags, float sigma, float clip,
                          float* out, float* normals, int32_t* face_index, void* stream);
/* Which form pcd_mesh_batch_clouds takes.  TEST / BENCHMARK ONLY: process-global.  1 (default): a slot's drawn cloud is kept in LDS
 * between the passes of the chain when num_points <= 8192 (96 KB) and drawn again from the counters in every pass above that;
 * 0: always drawn again.  Same bits either way.  PCD_ERR_ARG for any other code. */
int pcd_mesh_data_config(int code);

#ifdef __cplusplus
}
#endif
#endif /* PCD_HIP_H */
