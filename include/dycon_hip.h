/* libdycon_hip.so -- C ABI of the MI355X-native DyCON training-step kernels.
 *
 * The reference (rogeliorjr/DyCON_Paper_Replication) has no FFI: its hot path is plain
 * Python calling torch.nn / torch.nn.functional.  Each entry point below therefore cites the
 * reference call site (file:line under code/) whose ATen/cuDNN work it replaces; the Python
 * side (dycon_paper_replication_amd/) binds these with ctypes and mirrors the reference's
 * callables (net_factory_3d, UnCLoss, FeCLoss, losses.*, ramps.*).  See INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - activations are channels-last-3D: (B, D, H, W, C) contiguous, C fastest ("NDHWC");
 *   - dtype: DYCON_F32 or DYCON_BF16 storage; accumulation is always fp32;
 *   - outputs and workspaces are caller-allocated, no hidden allocation, no host sync:
 *     every call only enqueues work on `stream` and is hipGraph-capturable;
 *   - return 0 on success, <0 on error; dycon_last_error() gives a thread-local message.
 */
#ifndef DYCON_HIP_H
#define DYCON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* dycon_stream_t; /* == hipStream_t */

#define DYCON_F32 0
#define DYCON_BF16 1

#define DYCON_OK 0
#define DYCON_ERR_INVALID (-22)
#define DYCON_ERR_LAUNCH (-5)

/* gather modes of the convolution family */
#define DYCON_CONV_1X1 0  /* nn.Conv3d(k=1)          VNet.py:175, UNet3D_contrastive.py:249-250,262,265 */
#define DYCON_CONV_K3 1   /* nn.Conv3d(k=3, pad=1)   VNet.py:16, networks/utils.py:104,107              */
#define DYCON_CONV_K2S2 2 /* nn.Conv3d(k=2, stride=2) VNet.py:73                                          */

int dycon_version(void);
const char* dycon_last_error(void);

/* ---------------------------------------------------------------- weight packing
 * Reorders one fp32 weight tensor (torch layout, arbitrary strides) into the MFMA B-fragment
 * order consumed by dycon_conv_gemm:  K = T*Cin (tap-major, channel-minor), GEMM column
 * n = n1*N0 + n0.  Element (t, c, n1, n0) is read from w[t'*s_t + c*s_c + n1*s_n1 + n0*s_n0]
 * with t' = flip_taps ? T-1-t : t (flipped taps give the data-gradient of a k=3 conv).
 * Output bytes: dycon_bfrag_bytes(). */
size_t dycon_bfrag_bytes(int dtype, int T, int Cin, int N);
int dycon_pack_bfrag(const float* w, void* out, int dtype, int T, int Cin, int N, int N0,
                     long long s_t, long long s_c, long long s_n1, long long s_n0, int flip_taps,
                     dycon_stream_t stream);
/* Batched form: every pack of a training step in one launch.  jobs_dev is a DEVICE array of njobs descriptors
 * (built once -- the parameter arenas and packed buffers keep their addresses).  kind: 0 = bf16 fragments,
 * 1 = fp32 fragments, 2 = plain fp32 [T][Cin][N]; total = number of output elements; NT = ceil(N/16). */
typedef struct {
    const float* w;
    void* out;
    long long s_t, s_c, s_n1, s_n0, total;
    int kind, T, Cin, N, N0, flip, NT, pad_;
} dycon_pack_job_t;
int dycon_pack_batch(const dycon_pack_job_t* jobs_dev, int njobs, int blocks_per_job, dycon_stream_t stream);
/* plain fp32 [T][Cin][N] packing for the skinny (Cin<8 or N%16!=0) direct kernels */
int dycon_pack_tcn(const float* w, float* out, int T, int Cin, int N, int N0, long long s_t,
                   long long s_c, long long s_n1, long long s_n0, int flip_taps, dycon_stream_t stream);

/* ---------------------------------------------------------------- convolution family (implicit GEMM on MFMA)
 * y[row, n] (+)= bias[n % Cout] + sum_{t,c} x[src(row,t), c] * W[t, c, n]
 *   rows  = voxels of the output grid (mode 1x1/k3: the input grid; k2s2: the half grid)
 *   scatter=1: N = 8*Cout and column n = tap*Cout + co is written to output voxel
 *              2*row+tap of the doubled grid  == nn.ConvTranspose3d(k=2, s=2)  (VNet.py:100)
 *   accumulate=1: y += result (used to sum the two gradient paths into a skip tensor,
 *              VNet.py:210-222 / networks/utils.py:276).
 * Replaces F.conv3d / F.conv_transpose3d forward and their data-gradients.
 * Needs Cin % 8 == 0 (bf16) or Cin % 4 == 0 (f32), N % 16 == 0; otherwise use *_direct.
 * Exception (bf16, k3, >= 24^3 voxels): Cin == 1 with N in {16, 32, 64} (first layer) runs on the matrix cores
 * with wfrag packed as T=27, Cin=1 (K = 27 taps in one 32-wide k-step); Cin == 48 (U-Net
 * decoder) runs there with wfrag packed chunk-major: three T=27, Cin=16 packs of channels [0,16), [16,32),
 * [32,48) back to back.
 * workspace (optional, `workspace` bytes of the plan below): enables split-K for the small spatial
 * levels (6^3, 12^3), whose few row blocks cannot fill 256 CUs: per-split fp32 slabs + ordered finish.
 *
 * The plan.  Which kernel serves a shape, how many split-K slabs it leaves, the workspace it wants, whether it can take the
 * statistics of its output and which weight packing it reads is decided in ONE place (csrc/conv.hip, conv_fwd_plan); the launch and
 * every query below read that plan, and dycon_conv_gemm_plan hands it out (pure host code, no GPU needed):
 *   family    DYCON_CONV_*: the kernel family (DYCON_CONV_NONE: a shape dycon_conv_gemm refuses)
 *   splits    split-K slabs the caller sees (1: no workspace, no finish, defer_finish refused)
 *   workspace bytes of those slabs (0 when splits == 1)
 *   chunks    rows per sample of the statistics partials dycon_conv_gemm_stats writes (0: family cannot, or accumulate set)
 *   weights   DYCON_CONV_W_FRAG: one dycon_pack_bfrag pack; DYCON_CONV_W_CHUNK16: the chunk-major Cin == 48 packing above
 * dycon_conv_kernel_name gives the family's kernel name without the _kernel suffix; dycon_conv_region_name the name of one call
 * for a profile (the same, except conv_gemm_splitk for DYCON_CONV_GEMM with splits > 1: kernel + finish).  The three older queries
 * return one field each, and answer for a refused shape as they always have (the generic kernel's split plan). */
enum {
    DYCON_CONV_NONE = 0, DYCON_CONV_C1, DYCON_CONV_P16, DYCON_CONV_P32, DYCON_CONV_LDS, DYCON_CONV_HALO, DYCON_CONV_TILE,
    DYCON_CONV_GEMM
};
enum { DYCON_CONV_W_FRAG = 0, DYCON_CONV_W_CHUNK16 = 1 };
typedef struct {
    int family, splits, chunks, weights;
    size_t workspace;
} dycon_conv_plan_t;
int dycon_conv_gemm_plan(int dtype, int mode, int scatter, int accumulate, int B, int Di, int Hi, int Wi, int Cin, int N,
                         int Cout, dycon_conv_plan_t* plan);
const char* dycon_conv_kernel_name(int family);
const char* dycon_conv_region_name(const dycon_conv_plan_t* plan);
size_t dycon_conv_gemm_workspace(int dtype, int mode, int scatter, int B, int Di, int Hi, int Wi,
                                 int Cin, int N);
int dycon_conv_gemm(const void* x, const void* wfrag, const float* bias, void* y, int dtype,
                    int mode, int scatter, int accumulate, int B, int Di, int Hi, int Wi, int Cin,
                    int N, int Cout, float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* dycon_conv_gemm with defer_finish: on a split-K shape (plan splits > 1, workspace given, no accumulation; DYCON_ERR_INVALID otherwise) the
 * partial slabs stay in `workspace` ([split][row][N] fp32) and no finish is launched; the convolution is completed by
 * dycon_norm_fwd_slab, which fuses bias + ordered slab sum + rounding with the GroupNorm / InstanceNorm that follows
 * (VNet.py:16-23 at the 12^3 / 6^3 levels): one launch less on the step's critical chain, bit-identical results. */
int dycon_conv_gemm_splits(int dtype, int mode, int scatter, int B, int Di, int Hi, int Wi, int Cin, int N);
int dycon_conv_gemm_ex(const void* x, const void* wfrag, const float* bias, void* y, int dtype,
                       int mode, int scatter, int accumulate, int B, int Di, int Hi, int Wi, int Cin,
                       int N, int Cout, float* workspace, size_t ws_bytes, int defer_finish,
                       dycon_stream_t stream);
/* skinny channels (first layer 1->16, 1x1 heads 16->2 and their data-gradient 2->16):
 * w_tcn is fp32 [T][Cin][N]; x and y may have different dtypes (bf16 features, fp32 logits). */
int dycon_conv_direct(const void* x, int x_dtype, const float* w_tcn, const float* bias, void* y,
                      int y_dtype, int mode, int accumulate, int B, int Di, int Hi, int Wi, int Cin,
                      int N, dycon_stream_t stream);

/* weight gradient: dw[t*s_t + c*s_c + n*s_n] = sum_rows x[src(row,t), c] * gy[row, n]
 * (x on the input grid with Cin channels, gy on the output-row grid with Cout channels), and,
 * when dbias != NULL, the bias gradient dbias[n] = sum_rows gy[row, n] (fused into the same
 * pass over gy on the bf16 k=3 path).  Two-stage, deterministic: per-split partials in
 * `workspace`, then an ordered reduce. */
size_t dycon_conv_wgrad_workspace(int mode, int B, int Di, int Hi, int Wi, int Cin, int Cout);
/* the kernel dycon_conv_wgrad runs for these dtypes and this shape, named without the _kernel suffix (pure host code) */
const char* dycon_conv_wgrad_name(int x_dtype, int g_dtype, int mode, int B, int Di, int Hi, int Wi, int Cin, int Cout);
int dycon_conv_wgrad(const void* x, int x_dtype, const void* gy, int g_dtype, float* dw, float* dbias,
                     int mode, int B, int Di, int Hi, int Wi, int Cin, int Cout, long long s_t,
                     long long s_c, long long s_n, float* workspace, size_t ws_bytes,
                     dycon_stream_t stream);

/* out[c] = sum_rows x[row, c]   (bias gradients; also per-channel sums) */
size_t dycon_colsum_workspace(long long rows, int C);
int dycon_colsum(const void* x, int dtype, float* out, long long rows, int C, float* workspace,
                 size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- normalisation (+ReLU, + skip add)
 * One kernel family for nn.GroupNorm(16,C) (VNet.py:20), nn.InstanceNorm3d (G=C, no affine;
 * networks/utils.py:105,108) and train-mode nn.BatchNorm3d (Nb=1, G=C over all B*V rows;
 * UNet3D_contrastive.py:263,266).  x: (Nb, V, C).  stats: (Nb, G, 2) = {mean, rstd}. */
size_t dycon_norm_workspace(int Nb, long long V, int C);
int dycon_norm_stats(const void* x, int dtype, int Nb, long long V, int C, int G, float eps,
                     float* stats, float* running_mean, float* running_var, float momentum,
                     float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* statistics + apply in one call: ONE launch when V <= 2048 (12^3, 6^3 levels) (each workgroup owns whole groups of one sample),
 * otherwise dycon_norm_stats followed by dycon_norm_apply.  Same arguments as those two. */
int dycon_norm_fwd(const void* x, void* y, int dtype, int Nb, long long V, int C, int G, float eps,
                   float* stats, const float* gamma, const float* beta, int relu, const void* skip,
                   const float* chan_scale, float* running_mean, float* running_var, float momentum,
                   float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* 1 when dycon_norm_fwd serves this shape with its one-launch kernel (V <= 2048, whole groups per workgroup) */
int dycon_norm_fwd_is_fused(int dtype, long long V, int C, int G);
/* One-launch norm fed by the split-K slabs of the producing convolution (bf16 storage, shapes with dycon_norm_fwd_is_fused):
 * x_out = bf16(conv_bias + sum_z slab[z]) (kept for the backward), stats, y -- see dycon_conv_gemm_ex. */
int dycon_norm_fwd_slab(const float* slab, int splits, const float* conv_bias, void* x_out, void* y,
                        int dtype, int Nb, long long V, int C, int G, float eps, float* stats,
                        const float* gamma, const float* beta, int relu, const void* skip,
                        const float* chan_scale, dycon_stream_t stream);
/* y = act(gamma*(x-mean)*rstd + beta) * chan_scale[n,c] + skip ; gamma/beta/skip/chan_scale may be
 * NULL; y may alias x.  chan_scale (Nb, C) = keep/(1-p) fuses nn.Dropout3d (VNet.py:177,196,226). */
int dycon_norm_apply(const void* x, void* y, int dtype, int Nb, long long V, int C, int G,
                     const float* stats, const float* gamma, const float* beta, int relu,
                     const void* skip, const float* chan_scale, dycon_stream_t stream);
/* backward.  src = x (from_y=0, xhat=(x-mean)*rstd) or, ONLY when relu=0 (the op is then
 * invertible), y (from_y=1, xhat=(y-beta)/gamma).  gx may alias gy.  dgamma/dbeta may be NULL. */
int dycon_norm_bwd(const void* src, int from_y, const void* gy, void* gx, int dtype, int Nb,
                   long long V, int C, int G, const float* stats, const float* gamma,
                   const float* beta, int relu, const float* chan_scale, float* dgamma, float* dbeta,
                   float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* dycon_norm_bwd with defer_dparams = 1: on the one-launch shapes (dycon_norm_fwd_is_fused) the per-sample {dbeta, dgamma}
 * contributions stay in `workspace` ((Nb, C, 2) floats at its start) and the caller adds them up with dycon_norm_sum_dparams --
 * e.g. on the weight-gradient stream: the parameter gradients only feed the optimiser, the data gradient is the dependent chain.
 * Other shapes ignore the flag (their finalize launch writes dgamma / dbeta). */
int dycon_norm_bwd_ex(const void* src, int from_y, const void* gy, void* gx, int dtype, int Nb,
                      long long V, int C, int G, const float* stats, const float* gamma,
                      const float* beta, int relu, const float* chan_scale, float* dgamma, float* dbeta,
                      int defer_dparams, float* workspace, size_t ws_bytes, dycon_stream_t stream);
int dycon_norm_sum_dparams(const float* workspace, int Nb, int C, float* dgamma, float* dbeta,
                           dycon_stream_t stream);
/* The 2-class head fused into the V-Net's last normalisation (VNet.py:225-227: block_nine's conv -> norm -> ReLU [-> Dropout3d] ->
 * out_conv 1x1; train_DyCON_BraTS19.py:304).  C = 16 channels, 2 logits; head_w = out_conv.weight (2,16,1,1,1) fp32 as torch
 * stores it, head_b = out_conv.bias.  The normalised tensor and its gradient are never written:
 *   fwd : logits (Nb, V, 2) fp32 = head(act(norm(x)) * chan_scale), statistics from dycon_norm_stats
 *   bwd : gx = d/dx given g_logits (Nb, V, 2) fp32; dgamma / dbeta as dycon_norm_bwd; the head's weight / bias gradient partials
 *         stay in `workspace` (dycon_norm_head_workspace bytes) until dycon_norm_head_dparams sums them (any stream).
 * Per-voxel arithmetic and roundings are those of dycon_norm_apply + dycon_conv_direct (forward) and dycon_conv_direct's data
 * gradient + dycon_norm_bwd (backward): same logits bit for bit, same gx to fp32 round-off. */
size_t dycon_norm_head_workspace(int Nb, long long V);
int dycon_norm_head_fwd(const void* x, int dtype, int Nb, long long V, int G, const float* stats, const float* gamma,
                        const float* beta, int relu, const float* chan_scale, const float* head_w, const float* head_b,
                        float* logits, dycon_stream_t stream);
int dycon_norm_head_bwd(const void* x, const float* g_logits, void* gx, int dtype, int Nb, long long V, int G,
                        const float* stats, const float* gamma, const float* beta, int relu, const float* chan_scale,
                        const float* head_w, float* dgamma, float* dbeta, float* workspace, size_t ws_bytes,
                        dycon_stream_t stream);
int dycon_norm_head_dparams(const float* workspace, int Nb, long long V, float* d_head_w, float* d_head_b,
                            dycon_stream_t stream);
/* The same head for `classes` logits, 1..8 (net_factory_3d's class_num): logits / g_logits are (Nb, V, classes) fp32 rows,
 * head_w = out_conv.weight (classes,16,1,1,1), head_b = out_conv.bias.  Per voxel o_k = b_k, then o_k += y_c W[k][c] for c = 0..15;
 * gy_c = sum over k in order of g_k W[k][c], rounded to the storage type: the arithmetic of the launches the fusion replaces, so
 * the logits are theirs bit for bit.  classes = 2 is handed to the entry points above (same kernels, same bits).  The workspace holds classes * 17 head partials per
 * (sample, chunk) behind the normalisation's own. */
size_t dycon_norm_headc_workspace(int Nb, long long V, int classes);
int dycon_norm_headc_fwd(const void* x, int dtype, int Nb, long long V, int G, int classes, const float* stats,
                         const float* gamma, const float* beta, int relu, const float* chan_scale, const float* head_w,
                         const float* head_b, float* logits, dycon_stream_t stream);
int dycon_norm_headc_bwd(const void* x, const float* g_logits, void* gx, int dtype, int Nb, long long V, int G, int classes,
                         const float* stats, const float* gamma, const float* beta, int relu, const float* chan_scale,
                         const float* head_w, float* dgamma, float* dbeta, float* workspace, size_t ws_bytes,
                         dycon_stream_t stream);
int dycon_norm_headc_dparams(const float* workspace, int Nb, long long V, int classes, float* d_head_w, float* d_head_b,
                             dycon_stream_t stream);
/* The normalisation after the FIRST convolution (block_one, VNet.py:176) has one consumer of its data gradient: that convolution's
 * weight gradient (the image needs none).  So the gradient is never stored:
 *   dycon_norm_bwd_stats     = the first two launches of dycon_norm_bwd (statistics pass + finalize): dgamma / dbeta, and the per-group
 *                              {A, B} sums at float offset dycon_norm_bwd_ab_offset(Nb, V, C) of `workspace` (dycon_norm_workspace bytes);
 *   dycon_conv1_wgrad_normbwd = weight + bias gradient of a 1 -> 16 channel k=3 convolution (bf16) reading x (the image), gy (gradient
 *                              w.r.t. the normalisation's output) and z (its input); gz = norm-backward(gy, z) is formed per element on
 *                              load, rounded to bf16 as the stored tensor would have been.  dw layout as dycon_conv_wgrad.
 * Replaces the backward-apply pass (2 reads + 1 write of the step's largest tensor) and the weight gradient's read of its result. */
/* Statistics of a normalisation's input taken by the convolution that produces it.  On the shapes dycon_conv_stats_chunks serves (bf16
 * k=3 32 -> 32 on >= 1024 tiles: the persistent kernel of the 48^3 level) dycon_conv_gemm_stats is dycon_conv_gemm that also leaves
 * per-(sample, chunk, channel) {sum, sum of squares} of the values it STORED in stat_part ([B][chunks][Cout][2] floats); the
 * normalisation that follows is then dycon_norm_fwd_parts = finalize + apply, without the pass that re-reads the tensor
 * (BatchNorm: Nb = 1, chunks = B * chunks). */
int dycon_conv_stats_chunks(int dtype, int mode, int B, int Di, int Hi, int Wi, int Cin, int Cout);
/* (also served since round 3: the persistent kernels of the 96^3 level, bf16 k=3 16 -> 16 and 1 -> 16.)  dycon_norm_stats_parts is the
 * finalize alone (stats = mean / rstd per (n, g)), for consumers that apply the statistics themselves (dycon_norm_head_fwd). */
int dycon_norm_stats_parts(int dtype, int Nb, long long V, int C, int G, float eps, float* stats, float* running_mean,
                           float* running_var, float momentum, const float* part, int chunks, dycon_stream_t stream);
int dycon_conv_gemm_stats(const void* x, const void* wfrag, const float* bias, void* y, int dtype, int B, int Di, int Hi,
                          int Wi, int Cin, int Cout, float* stat_part, size_t stat_bytes, dycon_stream_t stream);
int dycon_norm_fwd_parts(const void* x, void* y, int dtype, int Nb, long long V, int C, int G, float eps, float* stats,
                         const float* gamma, const float* beta, int relu, const void* skip, const float* chan_scale,
                         float* running_mean, float* running_var, float momentum, const float* part, int chunks,
                         dycon_stream_t stream);
size_t dycon_norm_bwd_ab_offset(int Nb, long long V, int C);
int dycon_norm_bwd_stats(const void* src, const void* gy, int dtype, int Nb, long long V, int C, int G, const float* stats,
                         const float* gamma, const float* beta, int relu, const float* chan_scale, float* dgamma,
                         float* dbeta, float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* The whole backward of block_one in ONE pass over (x, z, gy): the normalisation's data gradient is affine in (g', z) with
 * coefficients that depend on group sums the same pass takes, so the first convolution's weight gradient is a combination of three tap
 * correlations (sum g' x, sum z x, sum x) that do not depend on them (csrc/conv.hip, first_block_bwd_kernel).  Writes dw / dbias of the
 * convolution (layout as dycon_conv_wgrad) and dgamma / dbeta of the normalisation; no bf16 rounding of the data gradient enters dw.
 * Replaces dycon_norm_bwd_stats + dycon_conv1_wgrad_normbwd (the inputs are read once instead of twice). */
size_t dycon_first_block_bwd_workspace(int B, int D, int H, int W);
int dycon_first_block_bwd(const void* x, const void* z, const void* gy, int B, int D, int H, int W, int Nb, int G,
                          const float* stats, const float* gamma, const float* beta, int relu, const float* chan_scale,
                          float* dgamma, float* dbeta, float* dw, float* dbias, long long s_t, long long s_c, long long s_n,
                          float* workspace, size_t ws_bytes, dycon_stream_t stream);
size_t dycon_conv1_wgrad_normbwd_workspace(int B, int D, int H, int W);
int dycon_conv1_wgrad_normbwd(const void* x, const void* z, const void* gy, int B, int D, int H, int W, int Nb, int G,
                              const float* stats, const float* gamma, const float* beta, int relu, const float* chan_scale,
                              const float* ab, float* dw, float* dbias, long long s_t, long long s_c, long long s_n,
                              float* workspace, size_t ws_bytes, dycon_stream_t stream);
/* Accumulator forms of dycon_norm_fwd / dycon_norm_bwd (from_y = 0): `acc` = dycon_norm_acc_doubles(Nb, V, C) doubles that are
 * ZERO on entry (a slice of an arena the caller clears once per step).  On the shapes that are not served by the one-launch kernels, every chunk of the
 * statistics pass adds its sums to acc (double atomics) and the apply pass forms the group statistics in its prologue: TWO launches
 * instead of three, forward (stats written for the backward, BatchNorm running statistics updated) and backward (dgamma / dbeta
 * written by the apply pass).  Same results up to the last bits of the double sums.  workspace: only used on the one-launch shapes. */
size_t dycon_norm_acc_doubles(int Nb, long long V, int C);
int dycon_norm_fwd_acc(const void* x, void* y, int dtype, int Nb, long long V, int C, int G, float eps,
                       float* stats, const float* gamma, const float* beta, int relu, const void* skip,
                       const float* chan_scale, float* running_mean, float* running_var, float momentum,
                       double* acc, dycon_stream_t stream);
int dycon_norm_bwd_acc(const void* src, const void* gy, void* gx, int dtype, int Nb, long long V, int C,
                       int G, const float* stats, const float* gamma, const float* beta, int relu,
                       const float* chan_scale, float* dgamma, float* dbeta, double* acc, float* workspace,
                       size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- data movement / pointwise
 * nn.MaxPool3d(2) (UNet3D_contrastive.py:225-237); idx holds the first-max position 0..7 */
int dycon_maxpool2_fwd(const void* x, void* y, uint8_t* idx, int dtype, int B, int D, int H, int W,
                       int C, dycon_stream_t stream);
int dycon_maxpool2_bwd(const void* gy, const uint8_t* idx, void* gx, int dtype, int B, int D, int H,
                       int W, int C, dycon_stream_t stream);
/* trilinear resize (networks/utils.py:264 align_corners=False; UNet3D_contrastive.py:309 True).
 * y/gy rows have `ldy` channels per voxel and the op touches channels [coff, coff+C): this is how
 * the decoder's torch.cat([skip, up]) (networks/utils.py:276) is written without a copy pass. */
int dycon_trilinear_fwd(const void* x, void* y, int dtype, int B, int Di, int Hi, int Wi, int Do,
                        int Ho, int Wo, int C, int ldy, int coff, int align_corners,
                        dycon_stream_t stream);
int dycon_trilinear_bwd(const void* gy, void* gx, int dtype, int B, int Di, int Hi, int Wi, int Do,
                        int Ho, int Wo, int C, int ldy, int coff, int align_corners,
                        dycon_stream_t stream);
/* Upsampling block's operator (networks/VNet.py:121-142): nn.Upsample(scale_factor=2, mode='trilinear', align_corners=False)
 * followed by nn.Conv3d(Cin, Cout, 3, padding=1), as ONE kernel:
 *   y = conv_k3_pad1(upsample_x2(x)) + bias,   x (B, Di, Hi, Wi, Cin) -> y (B, 2Di, 2Hi, 2Wi, Cout), NDHWC, fp32 or bf16 storage,
 * fp32 accumulation.  The zero padding of the convolution applies on the up-sampled grid; the up-sampled tensor is formed tile
 * by tile in LDS and never written to memory (csrc/upconv.hip).  wfrag: dycon_pack_bfrag(T = 27, Cin, N = Cout) of the Conv3d
 * weight, as for dycon_conv_gemm (k = tap * Cin + c).  bias may be NULL.
 * Channels: Cin 16, 48 or a multiple of 32; Cout a multiple of 16; anything else is DYCON_ERR_INVALID.  No workspace. */
int dycon_upconv_k3(const void* x, const void* wfrag, const float* bias, void* y, int dtype, int B,
                    int Di, int Hi, int Wi, int Cin, int Cout, dycon_stream_t stream);
/* dst[row, doff + c] = src[row, soff + c]  (concat / split of channel slices) */
int dycon_copy_channels(const void* src, int lds, int soff, void* dst, int ldd, int doff,
                        long long rows, int C, int dtype, dycon_stream_t stream);
/* ReLU of the V-Net's normalization='none' blocks (VNet.py:23-24, 87, 114), with the Dropout3d channel factor and the decoder's
 * skip add folded in like in the norm kernels: y = relu(z) * chan_scale[b, c] + skip; gz = (z > 0) * gy * chan_scale[b, c].
 * skip / chan_scale may be NULL. */
int dycon_relu_fwd(const void* z, const void* skip, const float* chan_scale, void* y, int dtype, int B, long long V, int C,
                   dycon_stream_t stream);
int dycon_relu_bwd(const void* z, const void* gy, const float* chan_scale, void* gz, int dtype, int B, long long V, int C,
                   dycon_stream_t stream);

/* y[b, v, c] = x[b, v, c] * scale[b, c]   (nn.Dropout3d(0.5), VNet.py:177,196,226; fwd and bwd) */
int dycon_scale_channels(const void* x, const float* scale, void* y, int dtype, int B, long long V,
                         int C, dycon_stream_t stream);
/* y = x * mask * inv_keep  with an explicit float keep-mask (parity tests) */
int dycon_mul_mask(const void* x, const float* mask, float inv_keep, void* y, int dtype,
                   long long n, dycon_stream_t stream);
/* Philox4x32-10 element-wise dropout (nn.Dropout(0.3), UNet3D_contrastive.py:253-254):
 * keep = u > p ; the same (seed, offset) regenerates the mask in backward */
int dycon_dropout_philox(const void* x, void* y, int dtype, long long n, float p, uint64_t seed,
                         uint64_t offset, dycon_stream_t stream);
/* scale[i] = bernoulli(1-p)/(1-p)  for i < n   (channel masks of Dropout3d) */
int dycon_channel_mask_philox(float* scale, long long n, float p, uint64_t seed, uint64_t offset,
                              dycon_stream_t stream);
/* y = x + clamp(N(0,1)*sigma, -clip, clip)   (train_DyCON_BraTS19.py:301-302); noise==NULL:
 * Philox + Box-Muller, else the explicit noise tensor is added (parity tests) */
int dycon_add_noise(const void* x, const float* noise, void* y, int dtype, long long n, float sigma,
                    float clip, uint64_t seed, uint64_t offset, dycon_stream_t stream);
int dycon_tanh(const void* x, int x_dtype, float* y, long long n, dycon_stream_t stream);
int dycon_cast(const void* x, int x_dtype, void* y, int y_dtype, long long n, dycon_stream_t stream);
/* y = a + b (b may be NULL -> copy) */
int dycon_add(const void* a, const void* b, void* y, int dtype, long long n, dycon_stream_t stream);

/* ---------------------------------------------------------------- voxel losses (2 classes)
 * One pass over student+teacher logits (fp32, (B,V,2)) and labels accumulates every sum the
 * step needs (train_DyCON_BraTS19.py:308-314,351-352; utils/losses.py:8-16,65-104,156-192;
 * utils/dycon_losses.py:94-118) into sums[16] (double, zeroed by the call):
 *   0 ce_sum   1 I1  2 Z1  3 Y1   4 I0  5 Z0  6 Y0   7 mse_sum  8 kl_sum  9 uncl_w  10 uncl_h
 * samples [0,LB) are labelled (CE, Dice), [LB,B) feed the consistency term, all feed UnCL.
 * fast != 0: hardware exp2 / log2 / rcp sequences (1-2 ulp) instead of the libm routines -- for
 * logits that come out of a bf16 network; the fp32 parity mode passes 0. */
int dycon_seg_losses_fwd(const float* s_logits, const float* t_logits, const void* labels,
                         int label_bytes, int B, int LB, long long V, float beta, double* sums,
                         int fast, dycon_stream_t stream);
/* g_logits = sum_k coef[k] * d(loss_k)/d(s_logits); coef (device, 5 floats): ce, dice_fg,
 * dice_multiclass, consistency (mse or kl per cons_kind), uncl -- already multiplied by the
 * upstream gradient.  Needs the sums from the forward call. */
int dycon_seg_losses_bwd(const float* s_logits, const float* t_logits, const void* labels,
                         int label_bytes, int B, int LB, long long V, float beta, const double* sums,
                         const float* coef, int cons_kind, float* g_logits, int fast,
                         dycon_stream_t stream);

/* vals[6] (device floats) = ce, dice(class 1), dice(mean over classes), cons mse, cons kl, uncl */
int dycon_seg_losses_finalize(const double* sums, int B, int LB, long long V, float beta, float* vals,
                              dycon_stream_t stream);
/* out[6] = total, ce, dice, cons, fecl, uncl with total = l_w*(ce+dice) + cons_w*cons + u_w*(fecl+uncl)
 * (train_DyCON_BraTS19.py:355-357); nonfinite[0] = !isfinite(total) (the NaN/Inf guard, :360-362).
 * dice_kind 0: class-1 dice, 1: multi-class; cons_kind 0: mse, 1: kl; fecl may be NULL. */
int dycon_step_loss(const float* vals, const float* fecl, float l_weight, float cons_weight,
                    float u_weight, int dice_kind, int cons_kind, float* out, int* nonfinite,
                    dycon_stream_t stream);
/* The same two reductions and the FeCL finalize (dycon_fecl_finalize) as ONE launch: the scalar end of the step's loss forward
 * from the raw accumulators -- sums (16 doubles of dycon_seg_losses_fwd) and fecl_out (4 doubles of dycon_fecl_fwd, may be NULL),
 * after a data-parallel run has all-reduced them (B, LB, fecl_rows are then the GLOBAL counts).  out[6] as dycon_step_loss. */
int dycon_step_losses(const double* sums, const double* fecl_out, int B, int LB, long long V, float beta,
                      double fecl_rows, float lambda_cross, int has_teacher, float l_weight, float cons_weight,
                      float u_weight, int dice_kind, int cons_kind, float* out, int* nonfinite,
                      dycon_stream_t stream);

/* ---------------------------------------------------------------- voxel losses (C classes, 2 <= classes <= 8)
 * The same pass for logits (B, V, classes) fp32 rows (channels-last, as the nets' heads write them); the 2-class entry points
 * above keep their code and bits.  sums holds dycon_seg_lossesc_nsums(classes) = 5 + 3 * classes doubles (zeroed by _fwd):
 *   0 ce_sum   1 mse_sum   2 kl_sum   3 uncl_w   4 uncl_h   5 + 3c: I_c  Z_c  Y_c   (c = 0 .. classes - 1)
 * with I_c = sum p_c [y == c], Z_c = sum p_c^2, Y_c = sum [y == c] over the labelled samples [0, LB), p = softmax(s_logits).
 *   ce          nn.CrossEntropyLoss()(logits[:LB], label[:LB].long())                      train_DyCON_BraTS19.py:313
 *   dice "fg"   losses.dice_loss(softmax[:LB, 1], label[:LB] == 1), class 1 only           train_DyCON_BraTS19.py:314, utils/losses.py:8-16
 *   dice "mc"   losses.DiceLoss(C)(softmax[:LB], label[:LB].unsqueeze(1)): mean over c of 1 - (2 I_c + s) / (Z_c + Y_c + s), s = 1e-5
 *                                                                                          train_DyCON_ISLES22.py:247, utils/losses.py:156-192
 *   mse / kl    softmax_mse_loss(p_s, p_t).mean() / softmax_kl_loss(p_s, p_t) on samples [LB, B): the reference passes PROBABILITIES,
 *               which these softmax again; both means run over (B - LB) V classes elements    utils/losses.py:65-104
 *   uncl        UnCLoss()(s_logits, t_logits, beta) on all B samples, log(p + 1e-6)         utils/dycon_losses.py:94-118
 * A label >= classes is a caller error; the kernels select by comparison and never index with it (such a voxel adds its
 * log-sum-exp to ce_sum and nothing to Y).
 * _fwd cons_kind: 0 accumulates mse_sum only, 1 kl_sum only, 2 both (the pass is bound by its exp / log sequences).
 * fast as dycon_seg_losses_fwd. */
int dycon_seg_lossesc_nsums(int classes);   /* 5 + 3 * classes; 0 for classes outside 2..8 */
int dycon_seg_lossesc_fwd(const float* s_logits, const float* t_logits, const void* labels, int label_bytes, int B, int LB,
                          long long V, int classes, float beta, int cons_kind, double* sums, int fast, dycon_stream_t stream);
/* g_logits = sum_k coef[k] * d(loss_k)/d(s_logits); coef (device, 5 floats) as dycon_seg_losses_bwd: ce, dice_fg, dice_multiclass,
 * consistency (cons_kind 0: mse, 1: kl), uncl.  Needs the sums of the forward call (the Dice ratios; after a data-parallel
 * exchange the global ones). */
int dycon_seg_lossesc_bwd(const float* s_logits, const float* t_logits, const void* labels, int label_bytes, int B, int LB,
                          long long V, int classes, float beta, const double* sums, const float* coef, int cons_kind,
                          float* g_logits, int fast, dycon_stream_t stream);
/* vals[6] as dycon_seg_losses_finalize: ce, dice(class 1), dice(mean over classes), cons mse, cons kl, uncl */
int dycon_seg_lossesc_finalize(const double* sums, int B, int LB, long long V, int classes, float beta, float* vals,
                               dycon_stream_t stream);
/* dycon_step_losses from the C-class accumulators (train_DyCON_BraTS19.py:355-362, train_DyCON_ISLES22.py:302-308): out[6] and
 * nonfinite as there; B, LB, fecl_rows are the GLOBAL counts after a data-parallel all-reduce of sums and fecl_out. */
int dycon_step_lossesc(const double* sums, const double* fecl_out, int B, int LB, long long V, int classes, float beta,
                       double fecl_rows, float lambda_cross, int has_teacher, float l_weight, float cons_weight,
                       float u_weight, int dice_kind, int cons_kind, float* out, int* nonfinite, dycon_stream_t stream);

/* ---------------------------------------------------------------- the reference's loss callables, reference semantics
 * The fused pass above takes LOGITS; the reference's own step body instead calls utils/losses.py on PROBABILITIES it computed
 * with torch (train_DyCON_BraTS19.py:308-314,352).  These entry points implement those callables literally, so that loop body
 * runs unchanged on this library.  All tensors are fp32 and described by a strided (n, C, V) view (element strides): channel
 * stride 1 for channels-last maps, V for plain NCDHW, element stride 2 for `probs[:, 1]`.  1 <= C <= 8. */
typedef struct {
    const void* p;          /* device pointer of element (0, 0, 0) */
    long long sn, sc, sv;   /* element strides of the sample, channel and (flattened) voxel index */
} dycon_view_t;
/* losses.softmax_mse_loss(a, b, sigmoid) (utils/losses.py:65-82): out = (softmax(a,1) - softmax(b,1))^2, element-wise */
int dycon_softmax_mse_fwd(const dycon_view_t* a, const dycon_view_t* b, const dycon_view_t* out, long long n, int C,
                          long long V, int sigmoid, dycon_stream_t stream);
/* ga = d sum(g * out) / d a  (the loss is symmetric: pass (b, a) for the gradient of the second argument) */
int dycon_softmax_mse_bwd(const dycon_view_t* a, const dycon_view_t* b, const dycon_view_t* g, const dycon_view_t* ga,
                          long long n, int C, long long V, int sigmoid, dycon_stream_t stream);
/* losses.softmax_kl_loss(a, b, sigmoid) (utils/losses.py:85-104) = F.kl_div(log_softmax(a,1), softmax(b,1), 'mean'):
 * out[0] = sum q (log q - log p) / (n C V); sum: one double of scratch (zeroed by the call). */
int dycon_softmax_kl_fwd(const dycon_view_t* a, const dycon_view_t* b, long long n, int C, long long V, int sigmoid,
                         double* sum, float* out, dycon_stream_t stream);
/* grad = g_up[0] * d out / d (which == 0 ? a : b) */
int dycon_softmax_kl_bwd(const dycon_view_t* a, const dycon_view_t* b, long long n, int C, long long V, int sigmoid,
                         int which, const float* g_up, const dycon_view_t* grad, dycon_stream_t stream);
/* losses.dice_loss(score, target) (utils/losses.py:8-16; C = 1, onehot = 0, target of the score's shape) and
 * losses.DiceLoss(C)(inputs, target, weight, softmax) (utils/losses.py:156-192; onehot = 1: target is the (n, V) label map,
 * class c's target is label == c):  out[0] = sum_c w_c (1 - (2 I_c + 1e-5)/(Z_c + Y_c + 1e-5)) / n_div, with the sums taken
 * over the WHOLE view (batch-global, as the reference).  target_kind: 0 float32, 1 one byte (uint8 / bool), 2 int64.
 * weights_host: C host floats or NULL (= 1).  sums: 24 doubles of scratch, kept for the backward. */
int dycon_dice_fwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, int onehot, long long n, int C,
                   long long V, int softmax, const float* weights_host, float n_div, double* sums, float* out,
                   dycon_stream_t stream);
int dycon_dice_bwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, int onehot, long long n, int C,
                   long long V, int softmax, const float* weights_host, float n_div, const double* sums, const float* g_up,
                   const dycon_view_t* grad, dycon_stream_t stream);

/* losses.dice_loss1(score, target) (utils/losses.py:19-27; softmax = 0, C = 1, target of the score's shape, any target_kind) and
 * losses.softmax_dice_loss(a, b) (utils/losses.py:39-56; softmax = 1: both views are logits, float32, and the softmax over the C
 * channels is taken inside):  out[0] = mean_c 1 - (2 sum s_c t_c + 1e-5) / (sum s_c + sum t_c + 1e-5), PLAIN sums over the whole
 * view.  sums: 24 doubles of scratch, kept for the backward. */
int dycon_dice1_fwd(const dycon_view_t* score, const dycon_view_t* target, int target_kind, long long n, int C, long long V,
                    int softmax, double* sums, float* out, dycon_stream_t stream);
/* grad = g_up[0] * d out / d a, the FIRST argument; the denominators are symmetric, so (b, a) with the same sums gives the second */
int dycon_dice1_bwd(const dycon_view_t* a, const dycon_view_t* b, int b_kind, long long n, int C, long long V, int softmax,
                    const double* sums, const float* g_up, const dycon_view_t* grad, dycon_stream_t stream);
/* H = -sum_c p_c log(p_c + 1e-6) over the C channels.  map != NULL: map[n V + v] = scale * H (losses.entropy_map, utils/losses.py:202-205;
 * entropy_loss_map, :59-62, with scale = 1 / log C); else out[0] = scale * mean H (entropy_minmization, :195-199; entropy_loss, :30-36)
 * with sum one double of scratch (zeroed by the call). */
int dycon_entropy_fwd(const dycon_view_t* p, long long n, int C, long long V, float scale, float* map, double* sum, float* out,
                      dycon_stream_t stream);
/* grad = d (sum g_map * map) / d p (g_map: n V floats) or g_up[0] * d out / d p; exactly one of g_map, g_up is non-NULL */
int dycon_entropy_bwd(const dycon_view_t* p, long long n, int C, long long V, float scale, const float* g_map, const float* g_up,
                      const dycon_view_t* grad, dycon_stream_t stream);
/* losses.symmetric_mse_loss(a, b) (utils/losses.py:107-116): out[0] = mean (a - b)^2 over count elements with element strides
 * a->sv, b->sv (sn, sc unused); sum: one double of scratch. */
int dycon_sym_mse_fwd(const dycon_view_t* a, const dycon_view_t* b, long long count, double* sum, float* out, dycon_stream_t stream);
/* grad = g_up[0] * d out / d a (pass (b, a) for the second argument) */
int dycon_sym_mse_bwd(const dycon_view_t* a, const dycon_view_t* b, long long count, const float* g_up, const dycon_view_t* grad,
                      dycon_stream_t stream);
/* losses.compute_kl_loss(a, b) (utils/losses.py:208-219): (kl_div(log_softmax(a,-1), softmax(b,-1), 'none').mean() + the same with a
 * and b exchanged) / 2, softmax over the LAST dimension: the views address n C V rows, row (in, ic, iv) at p + in sn + ic sc + iv sv,
 * of L elements with element stride sla / slb.  1 <= L <= 1024.  sum: one double of scratch. */
int dycon_kl_rows_fwd(const dycon_view_t* a, long long sla, const dycon_view_t* b, long long slb, long long n, long long C,
                      long long V, int L, double* sum, float* out, dycon_stream_t stream);
/* grad = g_up[0] * d out / d a (the loss is symmetric: pass (b, a) for the second argument); grad rows as the inputs', stride slg */
int dycon_kl_rows_bwd(const dycon_view_t* a, long long sla, const dycon_view_t* b, long long slb, long long n, long long C,
                      long long V, int L, const float* g_up, const dycon_view_t* grad, long long slg, dycon_stream_t stream);
/* losses.FocalLoss(gamma, alpha, size_average)(x, target) (utils/losses.py:119-153): out[0] = mean or sum over the n V voxels of
 * -(1 - pt)^gamma alpha[t] log pt, pt = softmax(x, 1)[t], t = target[n V + v] (contiguous; target_kind 1: uint8, 2: int64).
 * alpha_host: C host floats or NULL (= 1).  sum: one double of scratch. */
int dycon_focal_fwd(const dycon_view_t* x, const void* target, int target_kind, long long n, int C, long long V, float gamma,
                    const float* alpha_host, int size_average, double* sum, float* out, dycon_stream_t stream);
/* grad = g_up[0] * d out / d x with pt held constant, as the reference detaches it (utils/losses.py:141) */
int dycon_focal_bwd(const dycon_view_t* x, const void* target, int target_kind, long long n, int C, long long V, float gamma,
                    const float* alpha_host, int size_average, const float* g_up, const dycon_view_t* grad, dycon_stream_t stream);
/* dycon_losses.UnCLoss()(s, t, beta) for C classes (utils/dycon_losses.py:94-118): out[0] = mean over the n V voxels of
 * sum_c (p_c - q_c)^2 / (e^{beta H_s} + e^{beta H_t}) + beta (H_s + H_t), p = softmax(s, 1), q = softmax(t, 1),
 * H = -sum_c p_c log(p_c + 1e-6).  sum: one double of scratch.  (The DyCON step's 2-class UnCL is part of dycon_seg_losses_*.) */
int dycon_uncl_fwd(const dycon_view_t* s, const dycon_view_t* t, long long n, int C, long long V, float beta, double* sum, float* out,
                   dycon_stream_t stream);
/* grad = g_up[0] * d out / d s (the teacher logits t are constants) */
int dycon_uncl_bwd(const dycon_view_t* s, const dycon_view_t* t, long long n, int C, long long V, float beta, const float* g_up,
                   const dycon_view_t* grad, dycon_stream_t stream);

/* rows of (R, C): y = x / max(||x||, eps)   (F.normalize, train_DyCON_BraTS19.py:316-323) */
int dycon_l2norm_fwd(const void* x, void* y, float* norms, int dtype, long long R, int C, float eps,
                     dycon_stream_t stream);
int dycon_l2norm_bwd(const void* y, const float* norms, const void* gy, void* gx, int dtype,
                     long long R, int C, float eps, dycon_stream_t stream);
/* mask[b, n] = avg_pool3d(label, k) > 0.5   (train_DyCON_BraTS19.py:326-330) */
int dycon_mask_pool(const void* labels, int label_bytes, float* mask, int B, int D, int H, int W,
                    int kd, int kh, int kw, dycon_stream_t stream);

/* ---------------------------------------------------------------- FeCL (utils/dycon_losses.py:150-235)
 * Blockwise: the (B,N,N) similarity matrix is never materialised; Gram tiles are recomputed on
 * MFMA in each of the passes.  Columns are split over workgroups (partial row results in slabs,
 * combined in order on load): deterministic, and enough workgroups to fill the chip at N = 1728.  feat/teacher: (B,N,Dm) L2-normalised rows; mask: (B,N) float.
 * out (device, 4 doubles, zeroed by the call): student_sum, cross_num, cross_cnt, unused.
 * loss[0] (device float) = student_sum/(B*N) + lambda_cross*cross_num/(cross_cnt+1e-18). */
size_t dycon_fecl_workspace(int B, int N, int Dm);
int dycon_fecl_fwd(const void* feat, const void* teacher, const float* mask, const float* gambling,
                   int dtype, int B, int N, int Dm, float temperature, float gamma, int use_focal,
                   float cross_thresh, float lambda_cross, double* out, float* loss, float* workspace,
                   size_t ws_bytes, dycon_stream_t stream);
/* recompute loss[0] from `out` (after the sums were all-reduced across ranks); rows = global B*N */
int dycon_fecl_finalize(const double* out, double rows, float lambda_cross, int has_teacher, float* loss,
                        dycon_stream_t stream);
/* g_feat = coef[0] * d(loss)/d(feat); needs workspace and `out` untouched since the forward */
int dycon_fecl_bwd(const void* feat, const void* teacher, const float* mask, const float* gambling,
                   int dtype, int B, int N, int Dm, float temperature, float gamma, int use_focal,
                   float cross_thresh, float lambda_cross, const double* out, const float* coef,
                   void* g_feat, float* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- gambling-softmax uncertainty
 * (utils/dycon_losses.py:14-26 gambling_softmax, :209-211 the weighted student term; train_DyCON_Pancreas.py:242-246 the producer)
 * p = exp(l) / (sum_c exp(l_c) + 1e-18) with NO max shift (a logit above ~88.7 gives NaN, as in the reference).
 * x, y, gy, gx: (B, V, C) channels-last fp32, nvox = B*V, C in 1..8.  gx = dL/dx given gy = dL/dy and y = p. */
int dycon_gambling_softmax_fwd(const float* x, float* y, long long nvox, int C, dycon_stream_t stream);
int dycon_gambling_softmax_bwd(const float* y, const float* gy, float* gx, long long nvox, int C, dycon_stream_t stream);
/* u[b, n] = F.interpolate(H, scale_factor=1/k, trilinear, align_corners=False), H = -sum_c p_c log(p_c + 1e-6) of the 2-class
 * gambling softmax of logits (B, D, H, W, 2) fp32; k even per axis, n over the (D/kd, H/kh, W/kw) grid.  With an even k, u is the
 * mean of H over the 2x2x2 voxels {k i + k/2 - 1, k i + k/2} per axis.  fast: hardware exp / log / rcp (bf16 step).
 * _bwd ADDS gu[b, n] * du/dlogits into g_logits (same layout), touching the 8 voxels of each patch only. */
int dycon_gambling_uncertainty_fwd(const float* logits, int B, int D, int H, int W, int kd, int kh, int kw, float* u,
                                   int fast, dycon_stream_t stream);
int dycon_gambling_uncertainty_bwd(const float* logits, int B, int D, int H, int W, int kd, int kh, int kw,
                                   const float* gu, float* g_logits, int fast, dycon_stream_t stream);
/* FeCL with the uncertainty weight (utils/dycon_losses.py:209-211: focal result discarded, student term = mean(r * u)).
 * _fwd_rows: passes 1-3 of dycon_fecl_fwd with u = 1 and no focal weight, plus the per-row partial sums of sum_j ell_ij into
 * `rows` ([column split][B*N], dycon_fecl_rows_workspace bytes).  It does not write a loss.
 * _gambling_finalize (once u is known): r_i = sum_j ell_ij / (cnt_i - 1 + 1e-18) in a fixed order, out[0] = sum_i r_i u_i
 * (what dycon_step_losses / dycon_fecl_finalize read; u, r, gu hold B*N floats, rows is what _fwd_rows wrote), the gradient pass's row weights scaled by u in the workspace, and optionally
 * r (B*N) and gu = coef[0] * r / (B*N) = coef[0] * d(student term)/du.  Then dycon_fecl_bwd(gambling=NULL, use_focal=0) gives the
 * feature gradient.  _gambling_grad: gu = coef[0] * r / n. */
size_t dycon_fecl_rows_workspace(int B, int N, int Dm);
int dycon_fecl_fwd_rows(const void* feat, const void* teacher, const float* mask, float* rows, int dtype, int B, int N,
                        int Dm, float temperature, float cross_thresh, double* out, float* workspace, size_t ws_bytes,
                        size_t rows_bytes, dycon_stream_t stream);
int dycon_fecl_gambling_finalize(const float* u, const float* coef, int dtype, int B, int N, int Dm, double* out, float* r,
                                 float* gu, float* workspace, size_t ws_bytes, const float* rows, size_t rows_bytes,
                                 dycon_stream_t stream);
int dycon_fecl_gambling_grad(const float* r, const float* coef, long long n, float* gu, dycon_stream_t stream);

/* ---------------------------------------------------------------- optimiser (train_DyCON_BraTS19.py:155-164,268,369-372)
 * sumsq[0] += sum g^2 (double, caller zeroes) -> clip_grad_norm_; then one fused pass:
 *   coef = min(1, max_norm/(sqrt(sumsq)+1e-6)); g = coef*g + wd*p; m = mu*m + g; p -= lr*m   on [0,n_sgd)
 *   teacher = alpha*teacher + (1-alpha)*p                                                    on [0,n_all)
 * skip_flag (device int, may be NULL): non-zero -> leave everything untouched (NaN/Inf loss). */
int dycon_sumsq(const float* g, long long n, double* sumsq, dycon_stream_t stream);
int dycon_sgd_ema(float* p, const float* g, float* mom, float* teacher, long long n_sgd,
                  long long n_all, const double* sumsq, float max_norm, float grad_scale, float lr,
                  float momentum, float weight_decay, float ema_alpha, const int* skip_flag,
                  dycon_stream_t stream);
/* dst[i] = v_i for i < n <= 8: host scalars (loss weights) into device memory without a copy engine round trip */
int dycon_set_scalars(float* dst, int n, float v0, float v1, float v2, float v3, float v4, float v5,
                      float v6, float v7, dycon_stream_t stream);
/* flag[0] = !isfinite(x[0]) */
int dycon_nonfinite_flag(const float* x, int* flag, dycon_stream_t stream);

/* ---------------------------------------------------------------- sliding-window evaluation (code/utils/test_3d_patch.py:293-351)
 * score / cnt: fp32 maps of the (padded) volume D0 x D1 x D2, zeroed by the caller.  After a batch of n_patches <= 64 windows
 * went through the network, add for every voxel the class-1 softmax of each window covering it (logits: (n_patches, p0, p1, p2, 2)
 * fp32; origins_dev: n_patches x 3 ints, window corner in the volume) and the window count.  Voxel-centric, fixed window order:
 * deterministic although windows overlap.  This and the three other dycon_sw_accumulate* entry points launch one kernel
 * (csrc/sw_accumulate.h); class 1 of two logits is scored as 1 / (1 + exp(l0 - l1)) here. */
int dycon_sw_accumulate(const float* logits, int n_patches, int p0, int p1, int p2, const int* origins_dev,
                        float* score, float* cnt, int D0, int D1, int D2, dycon_stream_t stream);
/* the same for a C-class model, C in 2..8: logits (n_patches, p0, p1, p2, C) fp32; adds softmax(logits)[1] of the max-shifted C-way
 * softmax, for C == 2 too */
int dycon_sw_accumulate_c(const float* logits, int C, int n_patches, int p0, int p1, int p2, const int* origins_dev,
                          float* score, float* cnt, int D0, int D1, int D2, dycon_stream_t stream);
/* prob = score / cnt (may be NULL), label = prob > thresh   (:344-345) */
int dycon_sw_finalize(const float* score, const float* cnt, long long n, float thresh, uint8_t* label,
                      float* prob, dycon_stream_t stream);
/* out3 (device, caller zeroes) += { |pred|, |gt|, |pred & gt| }: the counts behind medpy.metric.binary.dc / jc
 * (test_3d_patch.py:496-508).  gt: uint8 (gt_bytes 1) or int64 (8), non-zero = foreground. */
int dycon_binary_overlap(const uint8_t* pred, const void* gt, int gt_bytes, long long n,
                         unsigned long long* out3, dycon_stream_t stream);

/* Train-time batch metrics (train_DyCON_BraTS19.py:385-392; utils/metrics.py compute_dice / compute_jaccard): for each sample b
 * out3b[3b..3b+2] (device, caller zeroes) += { |pred|, |gt|, |pred & gt| } with pred = softmax(logits)[1] > 0.5, read straight from
 * the (B, V, 2) fp32 logits. */
int dycon_batch_overlap(const float* logits, const void* gt, int gt_bytes, int B, long long V,
                        unsigned long long* out3b, dycon_stream_t stream);

/* ---------------------------------------------------------------- multi-class evaluation (csrc/evalc.hip)
 * The all-class form of the evaluator above (code/utils/test_3d_patch.py:334-336 computes the whole softmax; :337-347 keep class 1):
 * every window adds its C-way softmax, C in 2..8, to score, fp32 class-major (C, D0, D1, D2), and 1 to cnt (D0, D1, D2); logits
 * (n_patches, p0, p1, p2, C) fp32, n_patches <= 64.  Voxel-centric, fixed window order, no atomics.  The grid covers the box
 * [box_lo, box_hi) only (host ints; the bounding box of the chunk's windows, inside the volume); a voxel of the box that no window
 * of the chunk covers keeps its score and cnt. */
int dycon_sw_accumulate_all(const float* logits, int C, int n_patches, int p0, int p1, int p2, const int* origins_dev,
                            float* score, float* cnt, int D0, int D1, int D2, const int* box_lo, const int* box_hi,
                            dycon_stream_t stream);
/* p_c = score_c / cnt (code/utils/test_3d_patch.py:344), label = argmax_c p_c with the lowest index on ties (np.argmax); prob
 * (class-major (C, n), may be NULL, may be score itself) = p */
int dycon_sw_finalize_argmax(const float* score, const float* cnt, int C, long long n, uint8_t* label, float* prob,
                             dycon_stream_t stream);
/* label = argmax_c logits[v, c] of (nvox, C) fp32 logits, lowest index on ties: torch.argmax(softmax(outputs), dim=1) of
 * code/train_DyCON_ISLES22.py:364-366 */
int dycon_argmax_labels(const float* logits, int C, long long nvox, uint8_t* label, dycon_stream_t stream);
/* out (device, C*C + 1 counters, caller zeroes): out[p*C + g] += voxels with pred == p and gt == g, the counts behind the per-class
 * Dice of code/utils/metrics.py:14-27 (cal_dice) and medpy's dc / jc per class (code/utils/test_3d_patch.py:496-508); out[C*C] +=
 * voxels whose pred or gt lies outside [0, C), counted nowhere else.  gt: uint8 (gt_bytes 1) or int64 (8). */
int dycon_class_confusion(const uint8_t* pred, const void* gt, int gt_bytes, long long n, int C, unsigned long long* out,
                          dycon_stream_t stream);
/* The same per sample, out (B, C*C + 1), with pred = argmax_c logits read straight from the (B, V, C) fp32 logits: the C-class
 * form of dycon_batch_overlap (code/train_DyCON_BraTS19.py:385-392) */
int dycon_batch_class_confusion(const float* logits, const void* gt, int gt_bytes, int B, long long V, int C,
                                unsigned long long* out, dycon_stream_t stream);

/* ---------------------------------------------------------------- surface distances, unit voxel spacing (csrc/surface.hip)
 * HD95 / ASD of medpy.metric.binary (code/utils/test_3d_patch.py:496-508, code/utils/metrics.py:112-131) without a host copy.  A call
 * handles S = n_vol * n_cls pairs; pair s = v * n_cls + k reads volume v of a (prediction, uint8: a_bytes 1) and of b (ground truth,
 * uint8 or int64: b_bytes 1 or 8), each (n_vol, X, Y, Z) with Z innermost and every axis in 1..512.  Membership is voxel != 0 when
 * cls_lo == 0 (then n_cls must be 1), voxel == cls_lo + k otherwise.  Per pair and mask: border = m & ~erode6(m) with the outside of
 * the volume as background, then the exact int32 squared Euclidean distance transform of the border set in three separable passes.
 * hist (S, 2, nbins) unsigned int, nbins = (X-1)^2 + (Y-1)^2 + (Z-1)^2 + 1, zeroed by the call: hist[s][0][d] = border voxels of a at
 * squared distance d from the border of b, hist[s][1] the other direction; a direction whose target border is empty stays zero.
 * nborder (S, 2) = |border(a)|, |border(b)|.  Integer atomics only: the same bits on every run.  workspace: 2 int32 volumes per pair. */
size_t dycon_surface_workspace(int S, int X, int Y, int Z);
int dycon_surface_hist(const void* a, int a_bytes, const void* b, int b_bytes, int n_vol, int cls_lo, int n_cls, int X, int Y, int Z,
                       unsigned int* hist, unsigned int* nborder, void* workspace, size_t ws_bytes, dycon_stream_t stream);
/* out (S, 5) double = { percentile q of sqrt(bin) over both directions (np.percentile's default linear rule), mean a->b, mean b->a,
 * |border(a)|, |border(b)| }, fp64 in a fixed order, one workgroup per pair; the first three are NaN when either border is empty */
int dycon_surface_metrics(const unsigned int* hist, const unsigned int* nborder, int S, int nbins, double q, double* out,
                          dycon_stream_t stream);

/* ---------------------------------------------------------------- surface distances, any voxel spacing (csrc/surface_spacing.hip)
 * medpy's hd95 / asd with their voxelspacing and connectivity arguments.  a, b, n_vol, cls_lo, n_cls, X, Y, Z and the pair order are
 * those of dycon_surface_hist.  spacing: 3 host doubles for the axes X, Y, Z, read during the call, each finite, > 0 and within
 * 1e-150..1e150 (the squares stay normal numbers).  connectivity 1, 2, 3: border = m ^ erode(m) with 6, 18 or 26 neighbours, the
 * outside of the volume as background.  Per pair and mask the fp64 transform of the border set with the cost of an offset
 * (dx, dy, dz) = fl(fl(fl(wz dz^2) + fl(wy dy^2)) + fl(wx dx^2)), w = spacing^2, no contraction: the exact minimum of that cost,
 * whatever the grid.  out (S, 5) double as dycon_surface_metrics writes it: percentile q of both directions by a radix select over
 * the costs' bit patterns (np.percentile's default linear rule on their square roots), mean a->b and mean b->a as fp64 sums in an
 * order fixed by the shape, |border(a)|, |border(b)|; the first three are NaN when either border is empty.  Integer atomics only: the
 * same bits on every run.  No allocation, no host synchronisation.  workspace: dycon_surface_spaced_workspace bytes, 8-byte aligned
 * (2 fp64 volumes per pair and a fixed block of select state). */
size_t dycon_surface_spaced_workspace(int S, int X, int Y, int Z);
int dycon_surface_spaced_metrics(const void* a, int a_bytes, const void* b, int b_bytes, int n_vol, int cls_lo, int n_cls, int X, int Y,
                                 int Z, const double* spacing, int connectivity, double q, double* out, void* workspace,
                                 size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- 3-D connected components (csrc/components.hip)
 * The `nms` step of code/utils/test_3d_patch.py:19-26 (skimage.measure.label + the largest component) without a host copy.  vol:
 * (n_vol, X, Y, Z) uint8 or int64 (vol_bytes 1 or 8), Z innermost, every axis in 1..512, at most 65535 volumes and 2^31 - 1 voxels per
 * call.  connectivity 1, 2, 3 = 6, 18, 26 neighbours; neighbours never cross a face of a volume or the volumes of a batch.
 *   roots  : by_value == 0: a voxel is foreground when non-zero; by_value != 0: neighbours are connected only when their values are
 *            equal and lie in 1..255, every other value is background (skimage's rule on an integer map).  root (n_vol, X, Y, Z) int32
 *            = 0 for background, else 1 + the smallest linear index (x*Y + y)*Z + z of the voxel's component.  Three launches.
 *   labels : from root: labels int32 = 1..n in raster order of each component's first voxel (scipy.ndimage.label's numbering),
 *            ncomp (n_vol) = n.  A hierarchical scan (chunk counts, one workgroup per volume, fix-up); no workgroup waits on another.
 *   largest: from vol and its root: per volume (n_cls == 0, binary) or per volume and value 1..n_cls (n_cls >= 1, by value; other
 *            values give 0) the component of the greatest voxel count, the smallest root among equals.  out uint8 = 1 (binary) or the
 *            value on the winner, 0 elsewhere; win_size, win_root (n_vol, max(n_cls, 1)) int32, both 0 where there is no foreground.
 * Integer atomics only (atomicMin on parents, atomicAdd on sizes, a 64-bit atomicMax on (size << 32) | (0xFFFFFFFF - root)): the
 * same bits on every run.  No allocation, no host synchronisation, a fixed number of launches.  workspace: dycon_cc_workspace bytes
 * (one int32 per voxel plus small tables), used by labels and largest. */
size_t dycon_cc_workspace(int n_vol, int X, int Y, int Z);
int dycon_cc_roots(const void* vol, int vol_bytes, int n_vol, int X, int Y, int Z, int connectivity, int by_value, int* root,
                   dycon_stream_t stream);
int dycon_cc_labels(const int* root, int n_vol, int X, int Y, int Z, int* labels, int* ncomp, void* workspace, size_t ws_bytes,
                    dycon_stream_t stream);
int dycon_cc_largest(const void* vol, int vol_bytes, const int* root, int n_vol, int X, int Y, int Z, int n_cls, uint8_t* out,
                     int* win_size, int* win_root, void* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- lesion-wise statistics (csrc/lesions.hip)
 * From the root maps of a prediction and a ground truth to per-lesion sizes and overlaps and the per-volume detection counts behind
 * lesion-wise F1, lesion-count difference and volume difference.  root_pred, root_gt: (n_vol, X, Y, Z) int32 as dycon_cc_roots
 * writes them with by_value == 0 (0 = background, else 1 + the smallest linear index of the voxel's component inside its volume;
 * a value outside 1..X*Y*Z is read as background); shape limits are those of dycon_cc_roots.
 *   workspace: four sections of dycon_lesion_workspace / 4 bytes, each (n_vol, X*Y*Z) int32 addressed by root - 1 inside the volume:
 *            size of the prediction's lesions | their overlap | size of the ground truth's lesions | their overlap.  size = the voxel
 *            count of the component; overlap = the number of its voxels that are foreground in the other mask after the size filter
 *            (0 for a lesion the filter removes).  Entries that are no root are 0.
 *   filter : min_voxels >= 1.  A component of fewer voxels is removed from its own mask before anything else is counted, on both
 *            sides: a removed predicted lesion is no false positive and lends no overlap, a removed ground-truth lesion is no
 *            false negative.  Whole components go, so the survivors keep their roots.
 *   counts : (n_vol, 8) int64 over the surviving lesions: n_gt, n_pred (components), tp (ground-truth components with overlap > 0),
 *            fn (n_gt - tp), fp (predicted components with overlap == 0), vox_gt, vox_pred, vox_and (voxels of the two masks and
 *            of their intersection).  Overlap means shared voxels: lesions that only touch do not overlap, whatever the connectivity.
 * Integer atomics only, aggregated per wave (sizes, overlaps) and per workgroup (counts): the same bits on every run.  Two
 * hipMemsetAsync and three launches; no allocation, no host synchronisation, no workgroup waits on another. */
size_t dycon_lesion_workspace(int n_vol, int X, int Y, int Z);
int dycon_lesion_counts(const int* root_pred, const int* root_gt, int n_vol, int X, int Y, int Z, int min_voxels, long long* counts,
                        void* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- binary morphology on bit-packed masks (csrc/morphology.hip)
 * scipy.ndimage's binary_erosion / binary_dilation (hence opening and closing), binary_fill_holes and a component size filter, bit
 * for bit.  Shape limits are those of dycon_cc_roots: every axis 1..512, at most 65535 volumes and 2^31 - 1 voxels in one call.
 *   packed : a mask (n_vol, X, Y, Z) as (n_vol, X, Y, W) uint64 words, W = ceil(Z / 64): bit b of word w of a row is the voxel
 *            z = 64 w + b.  The bits z >= Z of a row's last word are 0 on entry and 0 after every operation.
 *   pack   : vol uint8 or int64 (vol_bytes 1 or 8).  by_value == 0: a voxel is foreground when non-zero; otherwise when it equals
 *            `value` (one class of a label map).  One wave ballot per word.
 *   unpack : out uint8 (n_vol, X, Y, Z), 0 / 1.
 *   stencil: `iterations` (1..64) erosions (op DYCON_MORPH_ERODE) or dilations (DYCON_MORPH_DILATE) by
 *            generate_binary_structure(3, connectivity), connectivity 1, 2, 3 = 6, 18, 26 neighbours and the centre.  Voxels outside
 *            the volume are background for both (scipy's border_value = 0).  The result is in `out`; `in` is left as it was;
 *            `scratch` (the size of `out`; may be NULL for iterations == 1) is the other buffer of the ping-pong.  The three must not
 *            overlap.  ceil(iterations / 4) launches: a workgroup stages 8 x 8 rows with a halo of up to 4 rows in LDS and runs up
 *            to 4 iterations there, one thread per word; nothing is unpacked in between.
 *   fill_holes: binary_fill_holes(mask, generate_binary_structure(3, connectivity)): the background is labelled with dycon_cc_roots at
 *            that connectivity, a background component with a voxel on one of the six faces is marked, out = mask | every voxel of an
 *            unmarked one.  workspace: dycon_morph_fill_workspace bytes.  Six launches and one hipMemsetAsync.
 *   dycon_cc_keep_min_size: from a root map of dycon_cc_roots (a value outside 1..X*Y*Z is background): out uint8 = 1 on the
 *            components of at least min_voxels (>= 1) voxels, 0 elsewhere.  workspace: dycon_cc_min_size_workspace bytes (one int32
 *            per voxel, the sizes addressed by root - 1).  Two launches and one hipMemsetAsync.
 *   merge_class: one step of the per-class recombination: where mask != 0, out = cls unless out already holds the voxel's own value
 *            of label_map (uint8 or int64).  Called for cls = C-1 .. 1 on a zeroed out, a voxel ends with its original class when that
 *            class's mask holds it, else with the smallest class whose mask does, else 0.
 * Integers only (the marks are plain stores of one value, the sizes integer atomics): the same bits on every run.  No allocation, no
 * host synchronisation, no workgroup waits on another. */
#define DYCON_MORPH_ERODE 0
#define DYCON_MORPH_DILATE 1
size_t dycon_morph_fill_workspace(int n_vol, int X, int Y, int Z);
size_t dycon_cc_min_size_workspace(int n_vol, int X, int Y, int Z);
int dycon_morph_pack(const void* vol, int vol_bytes, int n_vol, int X, int Y, int Z, int by_value, long long value, uint64_t* packed,
                     dycon_stream_t stream);
int dycon_morph_unpack(const uint64_t* packed, int n_vol, int X, int Y, int Z, uint8_t* out, dycon_stream_t stream);
int dycon_morph_stencil(const uint64_t* in, uint64_t* out, uint64_t* scratch, int n_vol, int X, int Y, int Z, int connectivity, int op,
                        int iterations, dycon_stream_t stream);
int dycon_morph_fill_holes(const uint64_t* mask, int n_vol, int X, int Y, int Z, int connectivity, uint64_t* out, void* workspace,
                           size_t ws_bytes, dycon_stream_t stream);
int dycon_cc_keep_min_size(const int* root, int n_vol, int X, int Y, int Z, int min_voxels, uint8_t* out, void* workspace,
                           size_t ws_bytes, dycon_stream_t stream);
int dycon_morph_merge_class(const void* label_map, int vol_bytes, const uint8_t* mask, int cls, long long n, uint8_t* out,
                            dycon_stream_t stream);

/* ---------------------------------------------------------------- signed distance maps (csrc/sdf.hip)
 * compute_sdf of code/utils/util.py:205-236 for S = n_vol * n_cls maps in one set of launches.  labels: (n_vol, X, Y, Z) uint8 or
 * int64 (label_bytes 1 or 8), Z innermost, every axis in 1..512.  Map s = v * n_cls + k takes volume v; its foreground is voxel != 0
 * when cls_lo == 0 (n_cls must be 1: the reference's astype(bool)), voxel == cls_lo + k otherwise (cls_lo + n_cls <= 256).
 * out: (S, n_rep, X, Y, Z) of out_bytes 4 (fp32) or 8 (fp64); the n_rep copies of a map are the reference's broadcast into an
 * output with a channel axis.  Per map, all in fp64 from exact int32 squared distances (util.py:219-232):
 *   no foreground voxel              +0.0 everywhere
 *   no background voxel              NaN everywhere (the reference's 0 / 0)
 *   foreground, squared distance to the background == 1     +0.0: the inner boundary of connectivity 1, which the faces of the
 *                                    volume do not create (not the border rule of dycon_surface_hist)
 *   other foreground voxels          -(sqrt(d2 to the background) / sqrt(max of it over the foreground))
 *   background voxels                +(sqrt(d2 to the foreground) / sqrt(max of it over the background))
 * normalize == 0 leaves the two divisions out: the signed distance in voxels with the same zeroed boundary and the same NaN rule.
 * An fp32 output is the fp64 value rounded once.  Unsigned integer atomicMax / atomicOr only: the same bits on every run.  One
 * hipMemsetAsync and at most five launches on the stream; no allocation, no host synchronisation.  workspace: 2 int32 volumes and
 * 4 unsigned words per map, 4-byte aligned. */
size_t dycon_sdf_workspace(int S, int X, int Y, int Z);
int dycon_sdf(const void* labels, int label_bytes, int n_vol, int cls_lo, int n_cls, int X, int Y, int Z, int normalize, int n_rep,
              int out_bytes, void* out, void* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- similarity monitor (utils/monitor.py:7-50)
 * The two histograms monitor_similarity_distributions draws, without the (B, N, N) similarity matrix: Gram tiles are recomputed
 * on MFMA in two sweeps (set ranges, then bins).  feat: (B, N, Dm) raw rows (dtype storage, Dm <= 256), normalised as F.normalize
 * (eps 1e-12); s_bij = <x_bi, x_bj> / tau; mask: (B, N) float, the pair is positive when mask[b,i] == mask[b,j] (the diagonal
 * included), negative otherwise; all B*N^2 ordered pairs, pooled over the batch.  Binning is np.histogram(values_f32, bins)'s:
 * range = float32 (min, max), +-0.5 when equal, (0, 1) when the set is empty; edge[k] = k*step + lo in float32 (no fma),
 * edge[bins] = hi.  Outputs (device): counts[2][bins] (pos, neg), edges[2][bins+1], minmax = pos lo, hi, neg lo, hi (the sets'
 * float32 extremes; 0, 1 for an empty set).  1 <= bins <= 256.  Bitwise reproducible; workspace O(B*N). */
size_t dycon_simhist_workspace(int B, int N, int Dm, int bins);
int dycon_simhist(const void* feat, const float* mask, int dtype, int B, int N, int Dm, float tau, int bins,
                  long long* counts, float* edges, float* minmax, float* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- 3-D ASPP (networks/assp.py:28-82; UNet3D(use_aspp=True))
 * The dilated k=3 convolutions run on dycon_conv_gemm (1x1 mode) over their live taps only: per axis of extent n the offsets +-d
 * can read data only if d < n (the caller plans the taps from the shape); their data gradient gathers the output gradient at
 * the negated offsets.  taps_host: ntaps (dz, dy, dx) triples, host memory.
 *   dycon_tap_gather : y (B,D,H,W, ntaps*C) = x shifted by each tap (zero outside the grid); C % 8 (bf16) / % 4 (f32) == 0
 *   dycon_pack_wblocks: MFMA B fragments (dycon_pack_bfrag order, T = 1, Cin = KB*kblk, N = NB*nblk) of a block table:
 *       block (kb, nb) = blk_host[kb*NB + nb] = src*32 + tap (or -1: zeros), element (k, n) of a block =
 *       w_host[src][tap + (k % kblk) * strides_host[2*src] + (n % nblk) * strides_host[2*src+1]]  (w_host: device pointers)
 *   dycon_unpack_wgrad: dense fp32 [KB*Ci][ldd] (column j*Co + co) -> g_host[j] (Co, Ci, taps_host[j] in {1, 27}) with
 *       g[co][ci][tap] = dense[(kb_host[j*27 + tap] * Ci + ci) * ldd + j*Co + co], or 0 where kb_host is -1 (pruned taps)
 *   dycon_sample_colsum: out[b][c] (+)= scale * sum_v x[b][v][c]      (global average pool; per-sample bias gradient)
 *   dycon_sample_bcast : y[b][v][c] = (x ? x[b][v][c] : 0) + scale * vec[b][c]   (x may alias y)
 *   dycon_small_gemm   : c[i*ldc + j] (+)= sum_r a[r*sar + i*sai] * b[r*sbr + j*sbj], fp32, r in order (pool-branch products)
 *   dycon_copy_segments: dst_host[k][0..n_host[k]) = src_host[k][...] for nseg <= DYCON_SEGS_MAX fp32 segments (device pointers)
 * All reject bad arguments before any launch and are bitwise reproducible. */
#define DYCON_TAPS_MAX 64
#define DYCON_WBLK_SRC_MAX 8
#define DYCON_WBLK_MAX 512
#define DYCON_SEGS_MAX 16
int dycon_tap_gather(const void* x, void* y, int dtype, int B, int D, int H, int W, int C, const int* taps_host, int ntaps,
                     dycon_stream_t stream);
int dycon_pack_wblocks(const float* const* w_host, const long long* strides_host, int nsrc, const short* blk_host, int KB, int NB,
                       int kblk, int nblk, void* out, size_t out_bytes, int dtype, dycon_stream_t stream);
int dycon_unpack_wgrad(const float* dense, long long ldd, int KB, float* const* g_host, const int* taps_host, const short* kb_host,
                       int ndst, int Ci, int Co, dycon_stream_t stream);
int dycon_sample_colsum(const void* x, int dtype, float* out, int B, long long V, int C, float scale, int accumulate,
                        dycon_stream_t stream);
int dycon_sample_bcast(const void* x, const float* vec, void* y, int dtype, int B, long long V, int C, float scale,
                       dycon_stream_t stream);
int dycon_small_gemm(const float* a, long long sar, long long sai, const float* b, long long sbr, long long sbj, float* c,
                     long long ldc, int I, int J, int R, int accumulate, dycon_stream_t stream);
int dycon_copy_segments(const float* const* src_host, float* const* dst_host, const int* n_host, int nseg, dycon_stream_t stream);

/* ---------------------------------------------------------------- training batches from a volume cache in HBM
 * (dataloaders/device_cache.py; the reference's RandomCrop -> RandomRotFlip -> ToTensor, code/dataloaders/brats19.py:198-283)
 * One launch writes out_image (njobs, 1, P0, P1, P2) fp32 and out_label (njobs, P0, P1, P2) uint8 (label_bytes 1) or int64
 * (label_bytes 8) from cached cases: `images` (fp32) and `labels` (uint8) are arenas, a case of stored shape (X, Y, Z) lies
 * C-contiguous at element offsets image_off / label_off.  Output sample n is
 *     flip(rot90(padded[ox+pad : ox+pad+P0, oy+pad : .., oz+pad : ..], k, axes (0, 1)), flip_axis)      (numpy semantics)
 * with the zero pad never materialised: (ox, oy, oz) is the crop origin in STORED coordinates (crop offset - pad, may be
 * negative) and every source index outside [0,X) x [0,Y) x [0,Z) reads as 0, image and label alike.  flip_axis -1: no flip.
 * jobs_host: njobs (1..DYCON_CROP_JOBS_MAX) descriptors in host memory, read at call time and passed to the kernel in its
 * arguments (nothing has to outlive the call).  The caller guarantees that every case lies inside its arena.  Rejected before
 * any launch: njobs out of range, a non-positive patch axis, k outside 0..3, flip_axis outside {-1, 0, 1}, an odd k with
 * P0 != P1 (the rotated crop would not have the patch's shape).  16-byte stores when P2 % 4 == 0 and the outputs are 16-byte
 * aligned, element stores otherwise; the source side assumes no alignment.  A pure gather: bitwise reproducible. */
#define DYCON_CROP_JOBS_MAX 16
typedef struct {
    long long image_off, label_off; /* element offsets of the case in the two arenas */
    int X, Y, Z;                    /* stored shape */
    int ox, oy, oz;                 /* crop origin, stored coordinates */
    int k;                          /* np.rot90 count, 0..3 */
    int flip_axis;                  /* -1 | 0 | 1 */
} dycon_crop_job_t;
int dycon_assemble_batch(const float* images, const uint8_t* labels, const dycon_crop_job_t* jobs_host, int njobs, int P0, int P1,
                         int P2, float* out_image, void* out_label, int label_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- model-ensemble sliding window (csrc/ensemble.hip;
 * code/utils/test_3d_patch.py:415-476, test_single_case_plus)
 * dycon_sw_gather: out (n, 1, p0, p1, p2) fp32 = windows [first, first + n) of a case, n in 1..64, in one launch.  vol: the UNPADDED
 * (w, h, d) fp32 volume; origins_dev: n_origins x 3 ints on the device, the window corners of the whole case in the coordinates of
 * the centre-padded volume (:418-439, :449-455: an axis shorter than the window is padded to it, (p - size) / 2 voxels in front).
 * The pad is index arithmetic: a source index outside the stored volume reads as 0, so out equals slicing the zero-padded volume bit
 * for bit and no origin can make the kernel read outside vol.  Rejected before any launch: a null pointer, a non-positive axis, n
 * outside 1..64, [first, first + n) outside the table. */
int dycon_sw_gather(const float* vol, int w, int h, int d, const int* origins_dev, int n_origins, int first, int n, int p0, int p1,
                    int p2, float* out, dycon_stream_t stream);
/* dycon_sw_accumulate for M = 2..4 models with C = 2..8 classes (:459-470): logits0..logits{M-1} are fp32 (n_patches, p0, p1, p2, C),
 * the rest is ignored (pass NULL).  Per covered voxel and class the logits are summed in model order, ((l0 + l1) + l2) + l3, and
 * divided by M ((y1_l + y1_r) / 2, :462); class 1 of the softmax of the mean is added to score and 1 to cnt, with the expression of
 * dycon_sw_accumulate for C == 2 and of dycon_sw_accumulate_c for C > 2 (one kernel body): the same model twice gives their bits
 * ((a + a) / 2 == a).
 * origins_dev: the n_patches x 3 corners of THIS chunk.  Voxel-centric, fixed window order, no atomics: deterministic. */
int dycon_sw_accumulate_ens(const float* logits0, const float* logits1, const float* logits2, const float* logits3, int M, int C,
                            int n_patches, int p0, int p1, int p2, const int* origins_dev, float* score, float* cnt, int D0, int D1,
                            int D2, dycon_stream_t stream);

/* ---------------------------------------------------------------- blended sliding window (csrc/ensemble.hip, csrc/sw_accumulate.h;
 * utils/sliding_window.py Blend).  Not in the reference: Gaussian importance weighting and mirror test-time augmentation.
 * An ENTRY is a window in one orientation: 4 ints (ox, oy, oz, mask), the corner as in dycon_sw_gather and bit a of mask set when the
 * window goes through the network flipped along window axis a (0, 1, 2 = dims 2, 3, 4 of the batch).  The table is device data and
 * is not validated: bits of mask above bit 2 are ignored, and no origin or mask can make a kernel read or write out of bounds.
 *
 * dycon_sw_gather_mirror: dycon_sw_gather for entries [first, first + n) of a table of n_entries x 4 ints on the device:
 * out[e, 0, i, j, k] = the zero-padded volume at (ox + (mask & 1 ? p0 - 1 - i : i), oy + (mask & 2 ? p1 - 1 - j : j),
 * oz + (mask & 4 ? p2 - 1 - k : k)).  Same conventions and the same checks; a pure copy: np.flip of the padded volume's slices, bit
 * for bit. */
int dycon_sw_gather_mirror(const float* vol, int w, int h, int d, const int* entries_dev, int n_entries, int first, int n, int p0,
                           int p1, int p2, float* out, dycon_stream_t stream);
/* The accumulate of dycon_sw_accumulate / _c / _ens / _all (one kernel body, csrc/sw_accumulate.h) for n <= 64 entries, entries_dev the
 * n x 4 ints of THIS chunk.  M in 1..4 models with logits0..logits{M-1} fp32 (n, p0, p1, p2, C), the rest NULL; C in 2..8.
 * all_classes 0: score (D0, D1, D2) receives class 1 of the softmax of the mean logits, by the two-logit expression for C == 2 and
 * the max-shifted softmax otherwise; all_classes 1 (needs M == 1): score is class-major (C, D0, D1, D2) and receives every class.
 * g0 / g1 / g2: device fp32 tables of p0 / p1 / p2 positive importances.  For every voxel of the box [box_lo, box_hi) (host int[3];
 * both NULL: the whole volume) and every entry of the chunk, in order, that covers it at local coordinate (la, lb, lc): the
 * probability p is formed from the logits at the mirrored coordinate (mask & 1 ? p0 - 1 - la : la, ...), which un-flips the
 * network's output, and with w = (g0[la] * g1[lb]) * g2[lc] in fp32 the voxel's sums take s += w * p (fused or not), n += w; then
 * score += s, cnt += n.  Voxel-centric, no atomics: deterministic.  Unit tables and mask 0 give the bits of the unweighted entry
 * points.  dycon_sw_finalize / dycon_sw_finalize_argmax divide as before. */
int dycon_sw_accumulate_weighted(const float* logits0, const float* logits1, const float* logits2, const float* logits3, int M, int C,
                                 int all_classes, int n, int p0, int p1, int p2, const int* entries_dev, const float* g0,
                                 const float* g1, const float* g2, float* score, float* cnt, int D0, int D1, int D2,
                                 const int* box_lo, const int* box_hi, dycon_stream_t stream);

/* ---------------------------------------------------------------- uncertainty maps and calibration (csrc/uncertainty.hip,
 * csrc/sw_accumulate.h; utils/uncertainty.py).  Not in the reference, whose evaluator keeps the mean softmax only
 * (code/utils/test_3d_patch.py:334-347); restated here are the textbook definitions over the MEMBERS of a voxel's ensemble, every
 * entry that covers it (window x orientation x model x Monte-Carlo pass), each with its own softmax p_e and weight w_e:
 *   H(p) = -sum_k p[k] ln p[k], a term with p[k] == 0 counting as 0 (saturated logits give entropy 0, never NaN).
 *
 * dycon_sw_accumulate_moments: dycon_sw_accumulate_weighted with M = 1, all_classes = 1 (same entries, tables, box, mirrored read,
 * fixed entry order, no atomics; score and cnt receive the same bits) that also adds, per voxel and covering entry,
 * w * H(p_e) to hsum (D0, D1, D2) and w * (p_e[k] * p_e[k]) to sq, class-major (C, D0, D1, D2).  All in fp32. */
int dycon_sw_accumulate_moments(const float* logits, int C, int n, int p0, int p1, int p2, const int* entries_dev, const float* g0,
                                const float* g1, const float* g2, float* score, float* cnt, float* hsum, float* sq, int D0, int D1,
                                int D2, const int* box_lo, const int* box_hi, dycon_stream_t stream);
/* Over n voxels: label and prob exactly as dycon_sw_finalize_argmax forms them (prob = score / cnt written over score, lowest index
 * on ties), and four fp32 maps of n values:
 *   entropy = H(prob)    expected_entropy = hsum / cnt    mutual_info = max(0, entropy - expected_entropy)
 *   variance = sum_k max(0, sq[k] / cnt - prob[k]^2) */
int dycon_sw_finalize_uncertainty(float* score, const float* cnt, const float* hsum, const float* sq, int C, long long n,
                                  uint8_t* label, float* entropy, float* expected_entropy, float* mutual_info, float* variance,
                                  dycon_stream_t stream);
/* The counts behind ECE / MCE (equal-width confidence bins, Guo et al. 2017), the Brier score, the negative log-likelihood and the
 * error-detection curves, of prob (C, V) fp32 class-major against label (V) uint8; mask (V) uint8, may be NULL: only voxels with
 * mask != 0 are scored.  K bins, 1..64.  Per scored voxel: confidence c = max_k prob[k], prediction = its first index, bin =
 * min(K - 1, (int)(c * (float)K)), the product one fp32 multiplication (never fused).
 *   counts (4K + 2 int64, device, zeroed here): n[K] | correct[K] | unc_hist[0][K] (correct voxels) | unc_hist[1][K] (wrong) |
 *           n_scored | scored voxels whose label lies outside [0, C), counted nowhere else (the rule of dycon_class_confusion)
 *   sums   (K + 2 fp64, device, written): conf_sum[K] = sum of c per bin | brier_sum = sum_v sum_k (prob[k] - [k == label])^2 |
 *           nll_sum = sum_v -ln max(prob[label], 1e-12); every term formed in fp64, nothing fused
 *   unc (V) fp32, may be NULL (the two histograms stay 0): an uncertainty per voxel with upper bound u_max > 0; its bin is
 *           min(K - 1, (int)(u / u_max * (float)K)), the division and the multiplication each rounded to fp32 in this order
 * A non-finite or negative binned value goes to bin 0.  Counts are integer atomics from per-wave LDS histograms; the fp64 sums are
 * per-workgroup partials in the workspace (fixed order inside a workgroup), folded by one workgroup in block order: no
 * floating-point atomic, the same bits on every run.  One hipMemsetAsync and two launches; no allocation, no host synchronisation.
 * workspace: 8-byte aligned, dycon_calibration_workspace(V, K) bytes (0 for arguments it rejects). */
size_t dycon_calibration_workspace(long long V, int K);
int dycon_calibration_counts(const float* prob, const uint8_t* label, const uint8_t* mask, const float* unc, float u_max, int C,
                             long long V, int K, long long* counts, double* sums, void* workspace, size_t ws_bytes,
                             dycon_stream_t stream);

/* ---------------------------------------------------------------- preprocessing: normalise and zoom (csrc/resample.hip;
 * code/BraTS19_DataPreprocessing.py:8-31, :175-198; code/ISLES22_DataPreprocessing.py:10-33, :141-159)
 * All volumes are C-contiguous fp32 (B, X, Y, Z) = B samples of V voxels, every sample with its own statistics.  NaN or infinite
 * input is out of scope: the results are then unspecified (never an out-of-bounds access).
 *
 * dycon_volume_stats: the scalars normalize_image (BraTS19_DataPreprocessing.py:8-31) takes from one volume, per sample:
 *   n_pos               voxels > 0 (:17 nonzero_mask)
 *   mean, std           fp64 mean and population standard deviation of those voxels (:19-20), two-pass: the mean first, then the
 *                       centred squares; 0 when n_pos == 0
 *   min_pos, max_pos    the smallest and the largest voxel > 0 (0 when there is none)
 *   min_all, max_all    the extremes over all voxels (what :25-26 read when the z-score is skipped)
 *   any_nonpos          1 when a voxel <= 0 exists
 * Sums are fp64 in a fixed order (per-workgroup partials in the workspace, folded by one workgroup: thread t takes partials t,
 * t + 256, ... in index order, then a fixed tree); counts and flags are integer
 * atomics; the extremes are integer atomicMax on the bit patterns of the floats (a minimum as the maximum of the complement).  No
 * floating-point atomic: the same bits on every run, for every alignment of x.
 * norm (may be NULL, as may stats, not both): the record normalize_image needs, derived without a second reduction:
 *   mean32, std32 = mean, std rounded once; apply_z = n_pos > 0 && std32 > 0 (:18, :21)
 *   apply_z:  lo32, hi32 = (min_pos - mean32) / std32, (max_pos - mean32) / std32 in fp32 (the z-score is monotone), widened by
 *             0.0f when any_nonpos (:22 puts 0 there)
 *   else:     lo32, hi32 = min_all, max_all (no voxel > 0, or std == 0: the raw values are min-maxed)
 *   apply_mm = hi32 > lo32 (:28; an all-zero volume, :13, has lo32 == hi32 == 0 and comes back unchanged)
 * One hipMemsetAsync and three launches on the stream; no allocation, no host synchronisation.  workspace: 8-byte aligned.
 *
 * dycon_normalize_apply: out = normalize_image(x) at full resolution given the records: per voxel, in fp32, each operation rounded
 * on its own (no fused multiply-add): z = x > 0 ? (x - mean32) / std32 : 0 when apply_z (:22), then (z - lo32) / (hi32 - lo32)
 * when apply_mm (:29).  out may alias x.
 *
 * dycon_zoom: scipy.ndimage.zoom(x, [Xo / X, Yo / Y, Zo / Z], order, mode="constant", cval=0, grid_mode=False) of every sample
 * (BraTS19_DataPreprocessing.py:190-194, ISLES22_DataPreprocessing.py:151-155), order 0 or 1.  Along an axis n_in -> n_out the
 * source coordinate of output index i is c = double(i) * (double(n_in - 1) / double(n_out - 1)) (0 when n_out == 1): IEEE doubles,
 * one multiplication, nothing fused.
 *   order 0   source index floor(c + 0.5) per axis, clamped to n_in - 1: a gather, bit for bit scipy's.  src fp32 -> out fp32
 *             or src uint8 -> out uint8 (src_bytes == out_bytes).  binarize != 0: out is uint8 and holds (float(value) > threshold)
 *             as 0 / 1, from an fp32 or a uint8 source: `(seg > 0).astype(np.uint8)` (BraTS :180) or `mask > 0.5` (ISLES :145)
 *             taken on load; the reference's `> 0.5` after the zoom (BraTS :198) then changes nothing.
 *   order 1   f = floor(c), t = c - f; eight taps in the order x, y, z with z fastest; a tap index beyond the last voxel is clamped
 *             (its weight is zero or rounding dust); weight (wx * wy) * wz with w = 1 - t or t; acc += weight * double(value)
 *             from 0.0, all in fp64, each multiplication and addition rounded on its own; rounded once to fp32 (out_bytes 4, what
 *             scipy returns for an fp32 input) or kept (out_bytes 8).  src fp32.  Differs from scipy by its summation order only.
 *   norm      (may be NULL; fp32 source, not with binarize) one record per sample: every tap value first goes through the two
 *             expressions of dycon_normalize_apply, so the full-resolution normalised volume is never written.
 * A first small launch writes the per-axis index / weight tables to the workspace, the second gathers: four consecutive z outputs
 * per thread, 16-byte stores (4-byte for uint8) when Zo % 4 == 0 and out is that aligned, element stores otherwise; the source
 * side assumes no alignment beyond the element's.  Rejected before any launch: a null pointer, an order outside {0, 1}, a
 * non-positive axis or batch, a type combination not listed above, a workspace smaller than dycon_zoom_workspace (0 for
 * arguments it rejects).  Bitwise reproducible. */
typedef struct {
    long long n_pos;
    double mean, std;
    float min_pos, max_pos, min_all, max_all;
    int any_nonpos, reserved;
} dycon_volume_stats_t;
typedef struct {
    int apply_z;
    float mean32, std32;
    int apply_mm;
    float lo32, hi32;
} dycon_norm_record_t;
size_t dycon_volume_stats_workspace(int B, long long V);
int dycon_volume_stats(const float* x, int B, long long V, dycon_volume_stats_t* stats, dycon_norm_record_t* norm, void* workspace,
                       size_t ws_bytes, dycon_stream_t stream);
int dycon_normalize_apply(const float* x, int B, long long V, const dycon_norm_record_t* norm, float* out, dycon_stream_t stream);
size_t dycon_zoom_workspace(int order, int Xo, int Yo, int Zo);
int dycon_zoom(const void* src, int src_bytes, int B, int X, int Y, int Z, int Xo, int Yo, int Zo, int order,
               const dycon_norm_record_t* norm, int binarize, float threshold, void* out, int out_bytes, void* workspace,
               size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- augmentation on the batch-assembly path (csrc/augment.hip;
 * dataloaders/device_augment.py; the reference's RandomRot and CreateOnehotLabel, code/dataloaders/isles22.py:24-28, :198-234)
 * dycon_assemble_batch_rot is dycon_assemble_batch with `scipy.ndimage.rotate(case, angle, order=0, reshape=False)` in front of
 * the chain and, optionally, the one-hot label written in the same launch.  The rotated volume never exists: the crop origin,
 * k and flip_axis of a job address the ROTATED volume (which keeps the stored shape), and for an output voxel whose index
 * (rx, ry, rz) into it lies inside [0,X) x [0,Y) x [0,Z) (outside: the reference's zero pad, 0) the source is found as scipy
 * finds it, in fp64, every operation rounded on its own (no fused multiply-add):
 *     cx = ((0.0 + rx * m[0]) + ry * m[1]) + off[0]          cy = ((0.0 + rx * m[2]) + ry * m[3]) + off[1]
 *     cx < 0 | cx > X - 1 | cy < 0 | cy > Y - 1  ->  0       (mode='constant': the test comes before the rounding)
 *     otherwise  stored[floor(cx + 0.5), floor(cy + 0.5), rz]
 * with m = [[c, s], [-s, c]] (c, s = cosdg, sindg of the angle) row-major and off = ctr - m @ ctr, ctr = ([X, Y] - 1) / 2, all
 * computed by the caller.  rotate == 0: m and off are ignored, (rx, ry) is the source, the bits are dycon_assemble_batch's.
 * out_onehot (may be NULL): (njobs, onehot_classes, P0, P1, P2) of element size onehot_bytes = 1 (uint8), 4 (fp32) or 8 (int64);
 * plane c holds label == c as 0 / 1, a label >= onehot_classes sets no plane; onehot_classes in 1..8.
 * Rejected before any launch: what dycon_assemble_batch rejects, a non-finite m / off of a rotating job, onehot_classes or
 * onehot_bytes out of range.  16-byte stores when P2 % 4 == 0 and every output is aligned for them, element stores otherwise.
 *
 * dycon_rotate_nearest: the same rotation of one whole C-contiguous (X, Y, Z) device volume of 1-, 4- or 8-byte elements into
 * `out` (which must not overlap `in`); it moves bytes, so any type of those sizes goes through.  m (4) and off (2) are host
 * pointers read at call time.  The source coordinates come from the same device function as the batch kernel's.
 * Both are pure gathers: bitwise reproducible. */
typedef struct {
    long long image_off, label_off; /* the fields of dycon_crop_job_t ... */
    int X, Y, Z;
    int ox, oy, oz;                 /* crop origin in the rotated volume (= stored coordinates) */
    int k;
    int flip_axis;
    double m[4];                    /* ... and the rotation: matrix, row-major */
    double off[2];                  /* offset */
    int rotate;                     /* 0: no rotation (m, off ignored) */
    int reserved;
} dycon_rot_job_t;
int dycon_assemble_batch_rot(const float* images, const uint8_t* labels, const dycon_rot_job_t* jobs_host, int njobs, int P0, int P1,
                             int P2, float* out_image, void* out_label, int label_bytes, void* out_onehot, int onehot_classes,
                             int onehot_bytes, dycon_stream_t stream);
int dycon_rotate_nearest(const void* in, void* out, int elem_bytes, int X, int Y, int Z, const double* m, const double* off,
                         dycon_stream_t stream);

/* ---------------------------------------------------------------- Gaussian filter (csrc/filters.hip; utils/filters.py)
 * dycon_gaussian_filter is scipy.ndimage.gaussian_filter of N C-contiguous fp32 volumes (X, Y, Z), bit for bit.  The caller forms the
 * weights as scipy does (fp64, r = int(truncate * sigma + 0.5), w = exp(-0.5 / sigma^2 * x^2) / sum for x = -r..r) and passes, per
 * axis, a HOST pointer to the 2 r + 1 of them, read at call time, or NULL for an axis scipy skips (sigma 0).  The axes are filtered
 * in the order 0, 1, 2, every intermediate is stored as fp32, and a line is summed in fp64 in scipy's symmetric form and order,
 *     acc = x[c] * w[r];   for ii = -r .. -1:  acc += (x[c + ii] + x[c - ii]) * w[ii + r];   out = (float)acc
 * with no fused multiply-add.  mode: how a line is extended (DYCON_FILTER_*; reflect wraps as often as r asks).  `scale` multiplies
 * the fp32 result of the last pass in fp32 (1: the filter alone, same bits).  r <= DYCON_GAUSS_RMAX on every axis; weights that are
 * not finite and exactly symmetric are rejected.  out == in filters in place; any other overlap is rejected.  The workspace holds
 * dycon_gaussian_filter_workspace(N, X, Y, Z, filtered axes, out == in) bytes.  No atomics: bitwise reproducible. */
#define DYCON_GAUSS_RMAX 64
#define DYCON_FILTER_REFLECT 0
#define DYCON_FILTER_CONSTANT 1
#define DYCON_FILTER_NEAREST 2
size_t dycon_gaussian_filter_workspace(int N, int X, int Y, int Z, int naxes, int inplace);
int dycon_gaussian_filter(const float* in, float* out, int N, int X, int Y, int Z, const double* w0, int r0, const double* w1, int r1,
                          const double* w2, int r2, int mode, float scale, void* workspace, size_t ws_bytes, dycon_stream_t stream);

/* ---------------------------------------------------------------- interpolating warp and intensity (csrc/warp.hip;
 * dataloaders/device_warp.py).  Not in the reference: the usual affine / elastic / intensity augmentations of 3-D segmentation,
 * computed as scipy.ndimage.affine_transform / map_coordinates (mode='constant', cval=0) compute them.
 * An output index (i0, i1, i2) has the source coordinate, in fp64, every operation rounded on its own (no fused multiply-add),
 *     c_d = (((0.0 + i0 * m[3 d]) + i1 * m[3 d + 1]) + i2 * m[3 d + 2]) + off[d]      [+ (double)displacement_d(i0, i1, i2)]
 * and the output is +0 unless 0 <= c_d <= n_d - 1 on all three axes.  Order 1: with f = floor(c), t = c - f, w0 = 1 - t and
 * w1 = 1 - w0 the eight corners are summed from 0.0 in the order (0,0,0), (0,0,1), (0,1,0) .. (1,1,1), each as
 * ((v[f + d] * wx) * wy) * wz, a corner at index n counting as 0, and the sum is rounded to the output type.  Order 0:
 * v[floor(c + 0.5)].
 *
 * dycon_assemble_batch_warp: dycon_assemble_batch_rot with that source.  An output voxel is taken back through flip_axis and k to
 * the patch index (a, b, z) as there; warp != 0: (i0, i1, i2) = (a, b, z), the image is read with the order-1 rule and the label with
 * the order-0 rule (the caller puts the crop origin into off); warp == 0: the source is (ox + a, oy + b, oz + z) and the bits are
 * dycon_assemble_batch's.  displacement (may be NULL): (njobs, 3, P0, P1, P2) fp32 on the device, read at (a, b, z) by the jobs
 * with elastic != 0 (which need warp != 0).  Labels, one-hot planes, alignment and rejections are dycon_assemble_batch_rot's.
 *
 * dycon_warp_volume: one C-contiguous (X, Y, Z) device volume -> (O0, O1, O2).  order 1: elem_bytes 4 (fp32) or 8 (fp64); order 0:
 * elem_bytes 1, 4 or 8, bytes are moved.  m (9, row-major) and off (3) are host pointers read at call time; displacement (may be
 * NULL): (3, O0, O1, O2) fp32 on the device.  `out` must not overlap `in`.
 *
 * dycon_intensity_augment: for i in 0..n-1 the V fp32 voxels of sample samples[i] (NULL: sample i) of x, with the five doubles
 * gain, bias, gamma, lo, hi = params[5 i ..] (host pointers, read at call time), in fp64, one rounding per operation:
 *     v = (double)x * gain + bias;  v = clip(v, lo, hi);  u = (v - lo) / (hi - lo);  [gamma != 1: u = pow(u, gamma);]
 *     y = (float)(u * (hi - lo) + lo)
 * gamma > 0 and lo < hi are required.  y == x works in place; samples that are not named are not touched.
 * All three are gathers or pointwise: no atomics, bitwise reproducible (pow is the device library's, not libm's). */
typedef struct {
    long long image_off, label_off; /* the fields of dycon_crop_job_t ... */
    int X, Y, Z;
    int ox, oy, oz;                 /* crop origin in stored coordinates (used when warp == 0) */
    int k;
    int flip_axis;
    double m[9];                    /* ... and the transform: matrix, row-major */
    double off[3];                  /* offset (holds the crop origin) */
    int warp;                       /* 0: the plain crop (m, off ignored) */
    int elastic;                    /* != 0: add the displacement (needs warp != 0) */
} dycon_warp_job_t;
int dycon_assemble_batch_warp(const float* images, const uint8_t* labels, const dycon_warp_job_t* jobs_host, int njobs,
                              const float* displacement, int P0, int P1, int P2, float* out_image, void* out_label, int label_bytes,
                              void* out_onehot, int onehot_classes, int onehot_bytes, dycon_stream_t stream);
int dycon_warp_volume(const void* in, int X, int Y, int Z, void* out, int O0, int O1, int O2, int order, int elem_bytes,
                      const double* m, const double* off, const float* displacement, dycon_stream_t stream);
int dycon_intensity_augment(const float* x, float* y, long long V, const long long* samples, const double* params, int n,
                            dycon_stream_t stream);

/* ---------------------------------------------------------------- per-kernel timing (bench.py `roofline`; diagnostics)
 * dycon_kernel_timing(1): from now on every kernel this library launches is bracketed by two HIP timing events on its launch
 * stream (earlier records are dropped); (0): stop.  Each LAUNCH is one record -- the finalize / reduce launch an entry point
 * enqueues after its main kernel is a record of its own.  _count: launches recorded so far (callers bracket an entry point by
 * reading it before and after the call).  _fetch: durations (ms), launch streams and kernel-name ids of records [first, first+n);
 * waits for those launches.  _name: the demangled kernel name of an id.  Not thread-safe; timing runs are single-threaded. */
int dycon_kernel_timing(int on);
long long dycon_kernel_timing_count(void);
int dycon_kernel_timing_fetch(long long first, long long n, float* ms, unsigned long long* stream, int* name_id);
const char* dycon_kernel_timing_name(int id);

#ifdef __cplusplus
}
#endif
#endif /* DYCON_HIP_H */
