/*
 * transvae_hip.h -- C ABI of libtransvae_hip.so, the gfx950 (MI355X) kernels
 * behind the TransVAE forward/backward path.
 *
 * The reference (benabbouosama/DEEPL-Project, R/ = transvae-implementation/)
 * has no FFI of its own: its hot path is a Python torch.nn.Module that
 * dispatches to stock ATen ops.  Each entry point
 * below therefore names the ATen call site(s) it replaces.  The Python shim in
 * deepl-project_amd/transvae/hip/ binds these with ctypes and raises
 * RuntimeError(tv_last_error()) on a non-zero status.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is
 *     allocated or freed inside, nothing synchronises the device
 *   - activations are bf16, NHWC (= token-major [B, H*W, C]), fp32 accumulate
 *   - gradients of parameters and all statistics are fp32
 *   - `stream` is a hipStream_t passed as void* (0 = default stream)
 *   - return value: 0 on success, TV_ERR_* otherwise
 */
#ifndef TRANSVAE_HIP_H
#define TRANSVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TV_OK 0
#define TV_ERR_ARG 1     /* bad shape / unsupported configuration */
#define TV_ERR_LAUNCH 2  /* HIP reported a launch error */
#define TV_ERR_INIT 3    /* no device / allocation of the zero page failed */
#define TV_ERR_UNSUPPORTED 4 /* tv_igemm_nt_cat2: this shape's tile has no two-source loop -- concatenate and call tv_igemm_nt (no error text);
                                tv_image_prep: an image outside the supported set (error text names it) */

#define TV_ACT_NONE 0
#define TV_ACT_GELU 1 /* exact (erf) GELU, R/transvae/modules/conv.py:56,86 */
#define TV_ACT_SILU 2 /* R/transvae/modules/upsample.py:35,96 */
/* Training-only variants of the saved tensor (no reference counterpart: autograd saves the pre-activation there).
 * desc.act | TV_ACT_SAVE_DERIV: `pre_act` receives act'(pre-activation) instead of the pre-activation, computed from the
 * same erf / exponential as the activation itself; tv_igemm_nt_actgrad(..., aux_act = TV_ACT_DERIV) then multiplies by
 * the saved tensor directly -- the backward epilogue carries no transcendental arithmetic. */
#define TV_ACT_DERIV 3
/* aux_act of tv_igemm_nt_actgrad only: the second tensor is ADDED, out = conv(x, w) + residual + aux -- two branch values
 * joining the residual stream in one fp32 sum with ONE rounding (the collapsed Conv-FFN tail: t + W_out u + (W_out W3) c,
 * R/transvae/modules/conv.py:85-104) */
#define TV_ACT_ADD 4
#define TV_ACT_SAVE_DERIV 16
/* ReLU, for the frozen VGG layers of the perceptual loss (tv_igemm_nt desc.act; aux_act of tv_igemm_nt_actgrad and act of
 * tv_act_bwd, where the "saved tensor" is the ReLU layer's own bf16 OUTPUT y and the factor is (y > 0) -- nothing else is
 * saved for such a layer, and pre_act must be NULL).  The name is deliberately outside the TV_ACT_ family, whose six ids
 * are pinned; csrc/common.h repeats it under the same name. */
#define TV_ACTX_RELU 5
/* LeakyReLU with the fixed slope 0.2 (the PatchGAN discriminator, csrc/gan.hip), under the same rules as TV_ACTX_RELU: as
 * desc.act nothing is saved (pre_act NULL); as aux_act / tv_act_bwd act the "saved tensor" is the layer's own bf16 OUTPUT y
 * (slope > 0, so sign(y) = sign(z)) and the factor is y > 0 ? 1 : 0.2. */
#define TV_ACTX_LRELU 6

/* library ------------------------------------------------------------------ */
int tv_init(void);                 /* allocates the device zero page; idempotent */
const char* tv_last_error(void);   /* message of the last failing call (thread local) */
int tv_abi_version(void);

/*
 * Geometry of one implicit-GEMM convolution / linear layer.
 *   x   : [batch, h_in, w_in, *] bf16, `ldx` elements between pixels (>= c_in)
 *   out : [batch, h_out, w_out, c_out] bf16, `ldo` elements between pixels
 * Virtual input coordinate of output (oy,ox), tap (ky,kx):
 *     uy = oy*stride + ky - pad ,  valid iff 0 <= uy < (h_in << up_shift)
 *                                        and (uy & dil_mask) == 0
 *     iy = uy >> up_shift                      (same for x)
 *   up_shift=1, dil_mask=0 : conv over a nearest-x2 upsampled input that is never
 *                            materialised (R/transvae/modules/upsample.py:94-95)
 *   up_shift=1, dil_mask=1 : zero-dilated input = data-gradient of a stride-2 conv
 * A linear layer is kh=kw=1, stride=1, pad=0, h=w=1, batch=#tokens.
 */
typedef struct tv_conv_desc {
    int batch, h_in, w_in, c_in, ldx;
    int h_out, w_out, c_out, ldo;
    int kh, kw, stride, pad;
    int up_shift, dil_mask;
    int act;           /* TV_ACT_* applied after bias, before residual */
    int store_shuffle; /* 1: pixel_shuffle(2) on store: out is [batch, 2*h_out, 2*w_out, c_out/4],
                          output column n = (dy*2+dx)*(c_out/4) + c  (upsample.py:121-123)
                          2: polyphase form of nearest-x2 upsample + 3x3 conv (upsample.py:94-95): the GEMM runs on the
                          (H+1) x (W+1) grid of 2x2 input neighbourhoods (kh = kw = 2, pad = 1, h_out = H+1, w_out = W+1),
                          column quadrant (py*2+px) of cell (y, x) is output pixel (2y - py, 2x - px) of the
                          [batch, 2H, 2W, c_out/4] result; phases that fall outside are dropped */
} tv_conv_desc;

/*
 * out = act(conv(x, w) + bias) + residual        (bf16 MFMA, fp32 accumulate)
 *   w        : [c_out, kh, kw, c_in] bf16 ("KRSC"; a Linear weight [out,in] is kh=kw=1)
 *   bias     : [c_out] fp32 or NULL
 *   residual : like out, or NULL
 *   pre_act  : like out, receives conv+bias before the activation (for backward), or NULL
 * Replaces F.conv2d / nn.Linear at R/transvae/modules/blocks.py:34,37, conv.py:39,54-60,65,
 * attention.py:43-48, upsample.py:33-37,42,93-98,103, the conv_in / conv_out / conv_mu / conv_logvar of models/{encoder,decoder,transvae}.py,
 * and -- called with rotated/transposed weights -- their data gradients.
 * Requires c_in % 32 == 0, c_out % 8 == 0, ldx % 8 == 0, ldo % 8 == 0 (bias, residual, pre_act, out 16-byte aligned).
 */
int tv_igemm_nt(const tv_conv_desc* d, const void* x, const void* w, const float* bias,
                const void* residual, void* pre_act, void* out, void* stream);

/* The QKV projection with RoPE in its epilogue (north star: "fused RMSNorm+RoPE+QKV-proj"; R/transvae/modules/attention.py:
 * 43-48 Linear q/k/v, :76-78 head split, :132-199 RoPE2D): out = x w^T + bias, and output columns < rope_cols (the q and k
 * thirds, whole heads of 64) are rotated with the table of tv_rope_qk before the single rounding to bf16; row m is token
 * m % tokens_per_image of its image. */
int tv_igemm_nt_rope(const tv_conv_desc* d, const void* x, const void* w, const float* bias, void* out,
                     const float* rope_tab, int tokens_per_image, int rope_cols, void* stream);

/*
 * Data gradient fused with the activation backward of the PREVIOUS layer:
 *     out = (conv(x, w) + residual) * act'(aux_pre_act)
 * i.e. the gradient w.r.t. the pre-activation tensor saved by the producing layer (aux_pre_act has the shape of
 * out).  Replaces autograd's GELU / SiLU backward (conv.py:56,86; upsample.py:35,96) without a separate pass.
 * aux_act = TV_ACT_ADD:  out = conv(x, w) + residual + aux_pre_act  (a second residual; see TV_ACT_ADD).
 */
int tv_igemm_nt_actgrad(const tv_conv_desc* d, const void* x, const void* w, const void* residual,
                        const void* aux_pre_act, int aux_act, void* out, void* stream);

/*
 * The same GEMM over K-CONCATENATED rows that are never materialised (1x1 / Linear geometry only, desc.c_in = k1 + k2):
 *     out = [x | x2] w^T (+ bias) (+ residual) (aux as in tv_igemm_nt_actgrad)
 * x supplies columns 0 .. k1-1 (row pitch desc.ldx), x2 columns k1 .. c_in-1 (row pitch ldx2); k1 and c_in - k1 multiples of 64;
 * w is [c_out][c_in] over the concatenated columns.  Two uses in the collapsed Conv-FFN tail (R/transvae/modules/conv.py:85-104):
 * t + [u | c] [W_out | W_out W3]^T and the data gradient onto u, [g | gz_c] [W_out ; W1] * gelu'.  Only the eight-phase loop of
 * the 256-row tiles has the second source: other shapes return TV_ERR_UNSUPPORTED (no error text) and the caller concatenates.
 */
int tv_igemm_nt_cat2(const tv_conv_desc* d, const void* x, const void* x2, int k1, int ldx2, const void* w, const float* bias,
                     const void* residual, const void* aux, int aux_act, void* out, void* stream);

/*
 * Weight gradient of the same layer (fp32):
 *   dw[co][ky][kx][ci] (+)= sum_p gy[p][co] * x_gathered[p][ky][kx][ci]
 *   dbias[co]          (+)= sum_p gy[p][co]                       (dbias may be NULL)
 *   gy : [batch, h_out, w_out, c_out] bf16 with `ldo` between pixels
 * The reduction over pixels is split over workgroups when the layer has few tiles; the partial tiles are then ADDED
 * into dw with fp32 atomics and the caller must pass a zeroed dw.  With a single pixel chunk every element of dw
 * is WRITTEN exactly once and dw needs no initialisation: tv_wgrad_tn_overwrites(d) says which of the two
 * tv_wgrad_tn will do for this geometry (1 = overwrites, 0 = accumulates, < 0 = bad descriptor).
 * dbias is ALWAYS added to (the workgroups that share a range of output channels take the pixel steps in turn and each
 * adds its share): pass it zeroed, or holding a running sum.
 * store_shuffle layers are handled by the caller as the transposed problem (x := the hi-res
 * gradient gathered with 2x2/stride-2 taps, gy := the layer input), so store_shuffle must be 0.
 * Requires c_in % 8 == 0, c_out % 8 == 0.
 * Replaces autograd's conv/linear weight-gradient for the call sites above.
 */
int tv_wgrad_tn(const tv_conv_desc* d, const void* x, const void* gy, float* dw, float* dbias,
                void* stream);
int tv_wgrad_tn_overwrites(const tv_conv_desc* d);
/* tv_wgrad_tn that always ADDS into dw / dbias (they hold the sum of earlier micro-batches): gradient accumulation without
 * autograd's separate add pass over 4.2 GB of gradients per micro-batch (R/train.py:557-646 accumulates through
 * loss.backward() into .grad). */
int tv_wgrad_tn_acc(const tv_conv_desc* d, const void* x, const void* gy, float* dw, float* dbias, void* stream);

/* Deterministic parameter gradients (csrc/det_reduce.hip): no atomics, the same bits on every run.
 * Every contributor of a sum STORES its partial result into a slice of its own in a caller-provided fp32 workspace; the
 * slice reduce then adds the slices in ascending index,
 *     S[i] = fl(...fl(fl(P_0[i] + P_1[i]) + P_2[i])... + P_{n_slices-1}[i]),   P_s = part + s * slice_stride,
 * and writes out[i] = S[i] (accum = 0) or fl(out[i] + S[i]) (accum = 1).  n >= 1 elements, slice_stride >= n. */
int tv_reduce_slices(const float* part, int n_slices, long long n, long long slice_stride, float* out, int accum,
                     void* stream);
/* The split of the deterministic weight gradient for this descriptor: *ny pixel chunks, and the workspace it needs,
 *     *workspace_bytes = ny * (c_out * kh * kw * c_in + c_out) * 4     with ny > 1   ([ny] weight slices, then [ny] bias slices)
 *     *workspace_bytes = 0                                             with ny == 1 (one block owns every tile: plain stores).
 * Host arithmetic only (no device is touched), the same answer on every call; `accum` changes neither number. */
int tv_wgrad_tn_plan(const tv_conv_desc* d, int accum, int* ny, long long* workspace_bytes);
/* tv_wgrad_tn (accum = 0: dw is written) / tv_wgrad_tn_acc (accum = 1: dw is added to) in deterministic form.  Chunk c's
 * tile goes to slice c of `workspace` (16-byte aligned), tv_reduce_slices adds the slices into dw in chunk order; dbias
 * -- always added to -- gets a slice per chunk the same way, summed by one workgroup per (chunk, 16 output channels).
 * Refuses (TV_ERR_ARG) a workspace smaller than tv_wgrad_tn_plan's answer.  dw needs no zeroing with accum = 0. */
int tv_wgrad_tn_det(const tv_conv_desc* d, const void* x, const void* gy, float* dw, float* dbias, int accum,
                    float* workspace, long long workspace_bytes, void* stream);

/*
 * fp32 -> bf16 weight repack.  src: [O, T, I] fp32 (T = kh*kw taps).
 *   dst   : [O, T, I] bf16 (forward operand)                      or NULL
 *   dst_t : [I, T, O] bf16 with taps reversed if flip_taps        or NULL
 *           (the operand of the data-gradient convolution)
 */
int tv_pack_weight(const float* src, void* dst, void* dst_t, int O, int T, int I, int flip_taps,
                   void* stream);

/* Operands DERIVED from a 3x3 weight by sums of taps, one launch each (replaces ~20-60 slice adds / copies of the host code):
 *   TV_DERIVE_UP_FWD         w fp32 [Cout,3,3,Cin] -> bf16 [4*Cout,2,2,Cin]: nn.Upsample(nearest, 2) + 3x3 conv
 *                            (R/transvae/modules/upsample.py:94-95) in polyphase form, row (2*py+px)*Cout + co, tap (ty,tx)
 *   TV_DERIVE_UP_DGRAD       w -> bf16 [Cin,4,4,Cout]: its adjoint, a 4x4 / stride-2 / pad-1 convolution of the high-resolution gradient
 *   TV_DERIVE_UP_WGRAD_FOLD  fp32 [Cin,4,4,Cout] (weight gradient of that adjoint) -> fp32 [Cout,3,3,Cin] (gradient of w);
 *                            accumulate != 0 adds into dst (gradient accumulation over micro-batches)
 *   TV_DERIVE_S2_PARITY      w -> bf16 [4*Cin,2,2,Cout]: data-gradient operand of the 3x3 / stride-2 convolution by output parity
 *                            (R/transvae/modules/upsample.py:33-37), taps outside a class's footprint zero
 * Sums are taken in fp32 in a fixed order (ky outer, kx inner) and rounded once. */
#define TV_DERIVE_UP_FWD 1
#define TV_DERIVE_UP_DGRAD 2
#define TV_DERIVE_UP_WGRAD_FOLD 3
#define TV_DERIVE_S2_PARITY 4
int tv_conv3x3_derived(const float* src, void* dst, int form, int c_out, int c_in, int accumulate, void* stream);

/* GroupNorm(32)+SiLU (R/transvae/modules/blocks.py:33,36,60-65; decoder.py:93,128-129) --------- */
/* Reductions over all pixels of an image span workgroups: each block writes a partial sum and a
 * finalize kernel adds the partials in block order (no atomics => bit-reproducible).  `partials`
 * is scratch of tv_gn_partial_count(batch, hw, C) floats. */
long long tv_gn_partial_count(int batch, int hw, int C);
/* per-(b,channel) sums about the pivot piv = x[b, pixel 0, c]: stats[b][c][0] = sum (x - piv), [1] = sum (x - piv)^2
 * (fp32; tv_gn_silu_fwd merges the channels of a group with Chan's (mean, M2) update -- no E[x^2] - mean^2 cancellation) */
int tv_gn_stats(const void* x, float* stats, float* partials, int batch, int hw, int C, void* stream);
/* y = silu(groupnorm(x)); stats from tv_gn_stats; writes mean/rstd per (b,group) to mr[b][G][2] */
int tv_gn_silu_fwd(const void* x, const float* stats, const float* gamma, const float* beta,
                   float* mr, void* y, int batch, int hw, int C, int G, float eps, void* stream);
/* y = silu(groupnorm(x)) again from the mean / rstd a tv_gn_silu_fwd call wrote to mr: the fused-op recompute of a
 * checkpointed ResBlock (R/transvae/models/encoder.py:97-99,117-118: activation checkpointing) -- bit-identical to the forward */
int tv_gn_silu_apply(const void* x, const float* mr, const float* gamma, const float* beta, void* y,
                     int batch, int hw, int C, int G, void* stream);
/* backward pass 1: red[b][c][0] = sum dh, red[b][c][1] = sum dh*xhat   (dh = dy * silu'(h)) */
int tv_gn_silu_bwd_reduce(const void* x, const void* dy, const float* mr, const float* gamma,
                          const float* beta, float* red, float* partials, int batch, int hw, int C,
                          int G, void* stream);
/* backward pass 2: dx (+= dres if given); dgamma/dbeta (fp32 [C]) accumulated from red with fp32 atomics -- or both null: the
 * parameter gradients are left to tv_gn_param_grads */
int tv_gn_silu_bwd_apply(const void* x, const void* dy, const void* dres, const float* mr,
                         const float* red, const float* gamma, const float* beta, void* dx,
                         float* dgamma, float* dbeta, int batch, int hw, int C, int G, void* stream);
/* deterministic parameter gradients of GroupNorm+SiLU from red [B][C][2] (tv_gn_silu_bwd_reduce): dbeta[c] += sum_b red[b][c][0],
 * dgamma[c] += sum_b red[b][c][1], the images added in b order */
int tv_gn_param_grads(const float* red, int B, int C, float* dgamma, float* dbeta, void* stream);

/* Token-wise norms (R/transvae/modules/blocks.py:179-194, attention.py:39-41,71-73) ------------
 * mode 0: y = x * rsqrt(mean(x^2)+eps_rms)                     (RMSNorm, weight folded downstream)
 * mode 1: u = x*w*rsqrt(mean(x^2)+eps_rms); y = (u-mean u)*rsqrt(var u + eps_ln)
 *         (RMSNorm followed by the affine-free LayerNorm shared by norm_q/k/v)
 * mode 2: y = (x-mean x)*rsqrt(var x + eps_ln)   (plain affine-free LayerNorm, forward only: the frozen ViT of the VF term)
 * rows: x,y [T, C] bf16; w fp32 [C] (mode 1 only). */
int tv_rownorm_fwd(const void* x, const float* w, void* y, int T, int C, int mode, float eps_rms,
                   float eps_ln, void* stream);
/* dx (+= dres if given) and, mode 1, dw[C] += ...  (fp32 atomics) */
int tv_rownorm_bwd(const void* x, const float* w, const void* dy, const void* dres, void* dx,
                   float* dw, int T, int C, int mode, float eps_rms, float eps_ln, void* stream);
/* tv_rownorm_bwd in deterministic form: each workgroup stores its partial weight gradient (its waves added in wave order) into
 * scratch[block][C], tv_reduce_slices adds the workgroups in order into dw (added to, as above).  The number of workgroups is a
 * function of (T, C) alone: tv_rownorm_bwd_det_scratch_bytes(T, C) is the scratch it needs; a smaller one is refused. */
long long tv_rownorm_bwd_det_scratch_bytes(int T, int C);
int tv_rownorm_bwd_det(const void* x, const float* w, const void* dy, const void* dres, void* dx, float* dw, int T,
                       int C, int mode, float eps_rms, float eps_ln, float* scratch, long long scratch_bytes,
                       void* stream);

/* RoPE (R/transvae/modules/attention.py:132-199), in place on the q and k thirds of
 * qkv [B, N, 3, heads, 64] bf16.  tab: [N, 4, 32] fp32 = cos1,sin1,cos2,sin2 per pair.
 * transpose=1 applies the adjoint (backward). */
int tv_rope_qk(void* qkv, const float* tab, int B, int N, int heads, int transpose, void* stream);

/* softmax(q k^T * scale) v, non-causal, head_dim 64 (attention.py:88-92).
 * qkv [B,N,3,heads,64] bf16; o [B,N,heads,64] bf16; lse [B,heads,N] fp32 (natural log). */
int tv_attn_fwd(const void* qkv, void* o, float* lse, int B, int N, int heads, float scale,
                void* stream);
/* dqkv [B,N,3,heads,64] bf16 from do; delta [2,B,heads,N] fp32 is scratch (the kernels keep -delta and -lse log2(e) there).  rope_tab (may be NULL): the table of tv_rope_qk;
 * when given, q and k in `qkv` are the ROTATED projections (tv_igemm_nt_rope) and dq / dk are stored as gradients w.r.t.
 * the un-rotated ones (the adjoint of attention.py:156-197 applied to the fp32 accumulators in the store). */
int tv_attn_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta,
                const float* rope_tab, void* dqkv, int B, int N, int heads, float scale, void* stream);

/* elementwise ------------------------------------------------------------------------------- */
/* dz = dy * act'(z)   (n bf16 elements, n % 8 == 0) */
int tv_act_bwd(const void* z, const void* dy, void* dz, long long n, int act, void* stream);
/* a += b (bf16, n % 8 == 0) */
int tv_add_(void* a, const void* b, long long n, void* stream);
/* NCHW fp32 [B,C,H,W] -> NHWC bf16 [B,H,W,Cpad] (channels >= C zero-filled) and back */
int tv_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int Cpad, void* stream);
int tv_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int Cpad, void* stream);
/* 3x3/pad-1 patches of an NCHW fp32 image -> [B*H*W, Kpad] bf16 rows ordered (ky,kx,c), for the
 * stem conv_in (R/transvae/models/encoder.py:52) */
int tv_im2col3x3(const float* src, void* dst, int B, int C, int H, int W, int Kpad, void* stream);
/* dst[b,y,x,c] = sum of the 2x2 block of src[b,2y+dy,2x+dx,c]  (adjoint of nearest x2) */
int tv_pool2x2_sum(const void* src, void* dst, int B, int H, int W, int C, void* stream);

/* Train-step glue around the path ------------------------------------------------------------------
 * Multi-tensor AdamW with the global-norm clip and the non-finite guard on the device, replacing the caller pattern
 *   clip_grad_norm_(model.parameters(), 1.0); optimizer.step()        (R/train.py:610-618, AdamW at :681-687)
 *   "skip the step when the loss is not finite"                       (R/train_2.py:328-338)
 * in two launches, plus one launch that refreshes every bf16 operand of the next forward / backward. */
typedef struct tv_opt_tensor {
    float* param;        /* fp32 master weights, updated in place */
    const float* grad;   /* fp32 gradient (same element order as param) */
    float* exp_avg;      /* Adam first moment  (fp32, updated in place) */
    float* exp_avg_sq;   /* Adam second moment (fp32, updated in place) */
    void* shadow_bf16;   /* optional: bf16 copy of param written by the update (NULL = none) */
    long long numel;
} tv_opt_tensor;
/* elements handled by one workgroup; chunk table = int pairs (tensor index, chunk index inside the tensor) */
int tv_opt_chunk_elems(void);
/* ctrl: 8 device floats owned by the caller, persistent across steps:
 *   [0] step count t   [1] gradient L2 norm   [2] clip coefficient   [3] 1 if this step is skipped (non-finite norm)
 *   [4] skipped steps so far   [5] 1 - beta1^t   [6] sqrt(1 - beta2^t)
 * Computes the global norm over all gradients (partials: n_chunks floats of scratch; fixed-order, bit-reproducible),
 * coef = min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping), advances t unless the norm is non-finite.
 * compute_norm = 0 skips the reduction (norm reported as 0, never skipped). */
int tv_opt_grad_norm(const tv_opt_tensor* table_dev, const int* chunks_dev, int n_chunks, float* partials,
                     float* ctrl, float max_norm, float beta1, float beta2, int compute_norm, void* stream);
/* AdamW update of every tensor in the table with g * ctrl[2] as the gradient; no-op when ctrl[3] != 0 */
int tv_opt_adamw(const tv_opt_tensor* table_dev, const int* chunks_dev, int n_chunks, const float* ctrl,
                 float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* shadow_bf16 = (bf16) param for every tensor that has one (first fill) */
int tv_opt_cast_shadows(const tv_opt_tensor* table_dev, const int* chunks_dev, int n_chunks, void* stream);
/* Exponential moving average of the weights, one launch over a table whose rows use `param` for the EMA tensor (fp32, updated in
 * place) and `grad` for the source weight (the other pointers are not read; NULL): ema = fmaf(a, w - ema, ema) with
 * a = one_minus_decay, which the caller forms as 1 - decay in fp64 and rounds once.  w == ema leaves the bits unchanged.  ctrl: NULL,
 * or the optimizer's control block: the launch is a no-op when ctrl[3] != 0 (that step was skipped).  Bound against fp64 with the
 * same fp32 a: 2 u (|w| + |ema|).  Rounding contract: DESIGN.md section 3.1 row S. */
int tv_opt_ema(const tv_opt_tensor* table_dev, const int* chunks_dev, int n_chunks, const float* ctrl, float one_minus_decay, void* stream);
/* every transposed operand in one launch: src bf16 [O,T,I] -> dst_t bf16 [I,T',O] (T' reversed if flip);
 * tile_start = exclusive prefix sum of ceil(O/64)*ceil(I/64)*T over the forms */
typedef struct tv_pack_form {
    const void* src;
    void* dst_t;
    int O, T, I, flip;
    long long tile_start;
} tv_pack_form;
int tv_pack_weight_multi(const tv_pack_form* forms_dev, int n_forms, long long total_tiles, void* stream);

/* Parameter folds ------------------------------------------------------------------------------------
 * A LayerNorm / RMSNorm affine in front of a Linear folds into the projection (attention.py:39-48,71-78; blocks.py:146-149):
 *   Wf[r][c] = W[r][c] * gamma[c],   bf[r] = sum_c W[r][c] * beta[c]     (beta / bf NULL together: no bias term)
 * and the gradients back onto W, gamma, beta in one pass (fp32, [R, C] row-major; column sums in a fixed order). */
int tv_fold_cols(const float* W, const float* gamma, const float* beta, float* Wf, float* bf, int R, int C, void* stream);
long long tv_fold_partial_count(int R, int C);     /* floats of scratch for tv_fold_cols_bwd */
int tv_fold_cols_bwd(const float* dWf, const float* dbf, const float* W, const float* gamma, const float* beta,
                     float* dW, float* dgamma, float* dbeta, float* partials, int R, int C, void* stream);

/* Closed-form loss terms on the path's outputs, value and gradient in one pass ---------------------
 *   out[0] = l1_weight * mean |f(recon) - target|     f = identity (R/transvae/losses/vae_loss.py:83-84) or sigmoid (P/...:80-84)
 *   out[1] = kl_weight * -0.5 * sum(1 + lv - mu^2 - exp(lv)) / kl_denom     (R/...:94-96: kl_denom = B*H_lat*W_lat;
 *            P/...:96-102: kl_denom = numel), lv = clamp(logvar, lo, hi) when lo < hi (R/train_2.py:316-318)
 *   out[2] = out[0] + out[1]
 * d_recon / d_mu / d_logvar (each may be NULL) receive the gradient of out[2]; all tensors fp32, any layout shared by the
 * tensors of a pair (they are walked flat).  partials: tv_vae_loss_partial_count(n_img, n_lat) floats of scratch. */
long long tv_vae_loss_partial_count(long long n_img, long long n_lat);
int tv_vae_loss_l1_kl(const float* recon, const float* target, const float* mu, const float* logvar,
                      float* d_recon, float* d_mu, float* d_logvar, float* partials, float* out,
                      long long n_img, long long n_lat, float l1_weight, float kl_weight, float kl_denom,
                      int sigmoid, float logvar_lo, float logvar_hi, void* stream);

/* Reconstruction metrics (evaluation, no gradient) -------------------------------------------------------------------------
 * Per-image MSE / PSNR / SSIM of a batch of fp32 pairs recon, target [B, C, H, W], each addressed through its own element
 * strides (n, c, h, w): NCHW-contiguous and channels_last tensors need no copy.  The input transform is applied first:
 *   TV_METRIC_CLIP    clamp both to [0, 1]                       (R/evaluate.py:109-110)
 *   TV_METRIC_SIGMOID sigmoid on recon only                      (P/evaluate_transvae.py:131)
 * SSIM window kinds (C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = data_range):
 *   TV_SSIM_SKIMAGE   skimage structural_similarity defaults (R/evaluate.py:116-120): 7x7 uniform, scipy 'reflect' border,
 *                     sample covariance (49/48), map cropped by 3 px, mean per channel then over channels; needs H, W >= 7
 *   TV_SSIM_BOX11     P/evaluate_transvae.py:56-77: 11x11 uniform, zero border divided by 121, population covariance,
 *                     mean over the whole map
 * out[0][b] = mse, out[1][b] = 10 log10(R^2 / mse) (+inf when mse == 0), out[2][b] = ssim, fp32 [3][B].
 * partials: tv_recon_metrics_partial_count(B, C, H, W, kind) floats of scratch (-1: bad arguments).  A stencil launch writes
 * one partial pair per tile, a finalise launch adds an image's partials in a fixed order in fp64 (no atomics: bit-reproducible,
 * independent of the rest of the batch). */
#define TV_SSIM_SKIMAGE 0
#define TV_SSIM_BOX11 1
#define TV_METRIC_NONE 0
#define TV_METRIC_CLIP 1
#define TV_METRIC_SIGMOID 2
long long tv_recon_metrics_partial_count(int B, int C, int H, int W, int kind);
int tv_recon_metrics(const float* recon, const float* target,
                     long long recon_sn, long long recon_sc, long long recon_sh, long long recon_sw,
                     long long target_sn, long long target_sc, long long target_sh, long long target_sw,
                     int B, int C, int H, int W, int kind, int transform, float data_range,
                     float* partials, float* out, void* stream);

/* LPIPS (VGG-16) perceptual term: everything that is not a convolution (csrc/lpips.hip) ---------------------------------------
 * The network is lpips.LPIPS(net='vgg') as R/transvae/losses/vae_loss.py:52,88-91 and R/evaluate.py:87-90,126-133 use it:
 * scaling layer, 13 3x3 convolutions + ReLU (tv_igemm_nt with TV_ACTX_RELU), four 2x2 max-pools, and on each of the five
 * taps relu{1_2,2_2,3_3,4_3,5_3} the head below.  Activations bf16 NHWC, sums fp32.
 *
 * 2x2 / stride-2 max-pool with floor semantics (F.max_pool2d(x, 2)): x [B, H, W, C] -> y [B, H/2, W/2, C], C % 8 == 0.
 * Backward recomputes the argmax from the saved input x (no index tensor) and routes gy to the FIRST maximum in torch's scan
 * order (rows, then columns; a later element wins only if greater or NaN), so it equals torch's backward bit for bit on ties:
 *     gx = route(gy) [+ add] [where x > 0, else 0]
 * add (or NULL): a second gradient of the same tensor, joined in one fp32 sum with one rounding; relu_mask != 0: x is a ReLU
 * output and gx is the gradient w.r.t. its pre-activation. */
int tv_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int C, void* stream);
int tv_maxpool2x2_bwd(const void* x, const void* gy, const void* add, void* gx, int B, int H, int W, int C, int relu_mask,
                      void* stream);
/* Input preparation: fp32 NCHW images [B, 3, H, W] -> cols [Ba + Bb, H, W, 32] bf16, the 3x3 / pad-1 patches ((ky, kx, c)
 * order, 27 of 32 used) of the scaled image, i.e. the operand of conv1_1 as a K = 32 GEMM.  Images 0 .. Ba-1 come from a with
 * flags_a, the other Bb from b with flags_b (b may be NULL when Bb == 0).  Per element, in this order:
 *   TV_LPIPS_SIGMOID  v = sigmoid(v)            (P/transvae/losses/vae_loss.py:80)
 *   TV_LPIPS_MAP      v = 2 v - 1               ([0, 1] -> [-1, 1]: normalize=True of lpips, vae_loss.py:88-89)
 *   TV_LPIPS_CLAMP    v = clamp(v, -1, 1)       (P/.../vae_loss.py:88-89)
 * then LPIPS's scaling layer (v - shift[c]) / scale[c]; shift_scale = {shift[3], scale[3]} fp32 on the device.
 * tv_lpips_prep_bwd is the adjoint for one source: dcols [B, H, W, 32] bf16 -> da [B, 3, H, W] fp32, the gradient w.r.t. a. */
#define TV_LPIPS_MAP 1
#define TV_LPIPS_SIGMOID 2
#define TV_LPIPS_CLAMP 4
int tv_lpips_prep(const float* a, const float* b, void* cols, int Ba, int Bb, int H, int W, int flags_a, int flags_b,
                  const float* shift_scale, void* stream);
int tv_lpips_prep_bwd(const void* dcols, const float* a, float* da, int B, int H, int W, int flags, const float* shift_scale,
                      void* stream);
/* Head of one tap.  feat [2B, HW, C] bf16: images 0 .. B-1 are x (reconstruction), B .. 2B-1 are t (target); w [C] fp32.
 *     f = x / (sqrt(sum_c x_c^2) + 1e-10), g likewise from t, d = sum_c w_c (f_c - g_c)^2, out[b] = mean over pixels of d
 * (accumulate != 0: out[b] += ..., the taps summed in call order).  grad (or NULL) [B, HW, C] bf16 receives
 * upstream / HW * dd/dx in the same launch; a pixel whose x is all zero gets a zero gradient.  C a power of two in [8, 512].
 * partials: tv_lpips_head_partial_count(B, HW, C) floats of scratch (-1: bad arguments); an image's partials are added in a
 * fixed order by a finalise launch, so out[b] is bit-reproducible and independent of the rest of the batch. */
long long tv_lpips_head_partial_count(int B, int HW, int C);
int tv_lpips_head(const void* feat, const float* w, float* partials, float* out, void* grad, int B, int HW, int C,
                  float upstream, int accumulate, void* stream);

/* The adversarial stage (csrc/gan.hip): a 70x70 PatchGAN discriminator and the GAN loss terms ----------------------------------
 * R/transvae/losses/vae_loss.py:103-111 (generator term), :199-244 (DiscriminatorLoss).  The reference ships no discriminator
 * network; the one built here is Conv(3,ndf,4,s2,p1)+LeakyReLU(0.2), three Conv(4x4, no bias)+BatchNorm+LeakyReLU blocks and
 * Conv(8 ndf,1,4,s1,p1).  Its convolutions are tv_igemm_nt / tv_wgrad_tn with kh = kw = 4; what follows is everything else.
 *
 * First-layer operand: fp32 image [B, 3, H, W] (element strides sn, sc, sh, sw: NCHW-contiguous and channels_last alike) ->
 * rows [B * H/2 * W/2, 64] bf16, the 4x4 / stride-2 / pad-1 patches in (ky, kx, c) order, column (ky*4 + kx)*3 + c, 48 of 64
 * used, the rest zero; sigmoid != 0 applies a sigmoid on read (P/transvae/losses/vae_loss.py:80,114-115).  Layer 0 is then a
 * K = 64 GEMM.  tv_patch4x4s2_bwd is the adjoint in gather form (each pixel sits in at most four patches; no atomics):
 * drows bf16 -> dimg fp32 [B, 3, H, W] contiguous, times sigmoid'(img) when the flag is set.  H, W even. */
int tv_patch4x4s2(const float* img, long long sn, long long sc, long long sh, long long sw, void* rows, int B, int H, int W,
                  int sigmoid, void* stream);
int tv_patch4x4s2_bwd(const void* drows, const float* img, long long sn, long long sc, long long sh, long long sw, float* dimg,
                      int B, int H, int W, int sigmoid, void* stream);
/* BatchNorm2d (training statistics over all M = B*H*W rows) + LeakyReLU(0.2) on rows x [M, C] bf16, C % 8 == 0, C <= 2048.
 * tv_bn_stats: per-channel sums of (x - piv) and (x - piv)^2 about the pivot piv = x[0][c], one partial per block
 * (tv_bn_partial_count(M, C) floats of scratch), added in a fixed order in fp64 by a finalise launch: bit-reproducible, no atomics.
 * Writes mr[0][c] = mean, mr[1][c] = 1 / sqrt(biased variance + eps), ss[0][c] = gamma*rstd, ss[1][c] = beta - mean*gamma*rstd, and
 * (running_mean / running_var not NULL) running = (1 - momentum) running + momentum {mean, M/(M-1) variance}.
 * tv_bn_lrelu_apply: y = lrelu(x * ss[0] + ss[1]) -- training forward, its recompute, and eval mode with ss built from the
 * running statistics.
 * tv_bn_lrelu_bwd_reduce: red[0][c] = sum dh, red[1][c] = sum dh * xhat with dh = dy * (x*ss[0] + ss[1] > 0 ? 1 : 0.2) and
 * xhat = (x - mr[0]) * mr[1], same fixed-order scheme; dbeta (+)= red[0], dgamma (+)= red[1] (accumulate != 0 adds).
 * tv_bn_lrelu_bwd_apply: dx = ss[0] * (dh - (red[0] + xhat red[1]) / M); eval_mode != 0: the plain affine dx = ss[0] * dh. */
long long tv_bn_partial_count(long long M, int C);
int tv_bn_stats(const void* x, const float* gamma, const float* beta, float* partials, float* mr, float* ss, float* running_mean,
                float* running_var, long long M, int C, float eps, float momentum, void* stream);
int tv_bn_lrelu_apply(const void* x, const float* ss, void* y, long long M, int C, void* stream);
int tv_bn_lrelu_bwd_reduce(const void* x, const void* dy, const float* mr, const float* ss, float* partials, float* red,
                           float* dgamma, float* dbeta, long long M, int C, int accumulate, void* stream);
int tv_bn_lrelu_bwd_apply(const void* x, const void* dy, const float* mr, const float* ss, const float* red, void* dx,
                          long long M, int C, int eval_mode, void* stream);
/* GAN loss terms on fp32 logits, value and gradient(s) in one pass.  a: n_a logits, b: n_b logits (NULL / 0 for TV_GAN_GEN).
 *   TV_GAN_GEN    out = weight * mean bce(a, 1)                          (the generator's term, vae_loss.py:106-111)
 *   TV_GAN_BCE    out = weight * (mean bce(a, 1) + mean bce(b, 0)) / 2   (a = real, b = fake; vae_loss.py:226-233)
 *   TV_GAN_HINGE  out = weight * (mean relu(1 - a) + mean relu(1 + b)) / 2
 *   TV_GAN_WGAN   out = weight * (-mean a + mean b)
 * bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)).  da / db (each may be NULL) receive d out / d a, d out / d b.  Block partials
 * (tv_gan_loss_partial_count(n_a, n_b) floats of scratch, 8-byte aligned: one fp64 partial per block -- the sums are carried in
 * fp64 from the first add, the wgan form being a difference of means) are added in block order by a finalise launch. */
#define TV_GAN_GEN 0
#define TV_GAN_BCE 1
#define TV_GAN_HINGE 2
#define TV_GAN_WGAN 3
long long tv_gan_loss_partial_count(long long n_a, long long n_b);
int tv_gan_loss(const float* a, const float* b, float* da, float* db, float* partials, float* out, long long n_a, long long n_b,
                int mode, float weight, void* stream);

/* rFID: everything of the FID Inception-v3 pool3 extractor that is not a convolution, and the Frechet statistics (csrc/fid.hip) --
 * The network is the FID literature's Inception-v3 (pt_inception / pytorch-fid FIDInceptionV3): input in [0, 1], bilinear resize
 * to 299 x 299 (align_corners=False, no antialiasing), 2x - 1, 94 bias-free convolutions with eval-mode BatchNorm (folded into
 * the bf16 weight and an fp32 bias at pack time) and ReLU -- tv_igemm_nt launches with TV_ACTX_RELU --, 3x3 pools, global
 * average pool -> [B, 2048] fp32.  Activations bf16 NHWC.
 *
 * tv_fid_prep: fp32 NCHW images a [Ba, 3, H, W] and b [Bb, 3, H, W] (b may be NULL with Bb = 0), H, W >= 8 -> cols
 * [Ba + Bb, 149, 149, 32] bf16: the 3x3 / stride-2 / unpadded patches ((ky, kx, c) order, 27 of 32 columns used, the rest zero)
 * of the resized, 2x - 1 mapped image, i.e. the operand of the first convolution as a K = 32 GEMM.  clip != 0 clamps the source
 * pixels to [0, 1] first.  The interpolation weights are exact fractions rounded once to fp32. */
int tv_fid_prep(const float* a, const float* b, void* cols, int Ba, int Bb, int H, int W, int clip, void* stream);
/* 3x3 pools, x [B, H, W, C] bf16 -> y [B, Ho, Wo, *] with row stride ldo >= C (a column range of a wider tensor), C % 8 == 0:
 *   TV_POOL3_MAX_S2     max, stride 2, no padding, Ho = (H - 3) / 2 + 1       (bit-equal to F.max_pool2d(x, 3, 2))
 *   TV_POOL3_MAX_S1P1   max, stride 1, pad 1                                  (bit-equal to F.max_pool2d(x, 3, 1, 1))
 *   TV_POOL3_AVG_S1P1   average, stride 1, pad 1, divided by the number of in-bounds taps (count_include_pad=False): fp32 sum in
 *                       tap order, one IEEE division, one rounding to bf16 */
#define TV_POOL3_MAX_S2 0
#define TV_POOL3_MAX_S1P1 1
#define TV_POOL3_AVG_S1P1 2
int tv_pool3x3(const void* x, void* y, int B, int H, int W, int C, int ldo, int mode, void* stream);
/* Row gather along one axis: x [B, H, W, C] bf16 -> y [B * H * W, taps * C] bf16 with
 * y[(b, i, j), t, c] = x[b, i + t - taps / 2, j, c] (axis 0) or x[b, i, j + t - taps / 2, c] (axis 1), zero outside the image.
 * taps is 3 or 7, C % 8 == 0.  A 1 x taps / taps x 1 "same" convolution is then a GEMM with K = taps * C (the descriptor of
 * tv_igemm_nt has one pad for both axes and cannot express it). */
int tv_gather_line(const void* x, void* y, int B, int H, int W, int C, int taps, int axis, void* stream);
/* Global average pool: x [B, HW, C] bf16 -> out [B, C] fp32; pixels summed in order in fp64, one rounding.  C % 8 == 0. */
int tv_global_avgpool(const void* x, float* out, int B, int HW, int C, void* stream);
/* Spatial feature rows (sFID): x [B, HW, ldc] bf16 with C <= ldc channels per position -> out [B, ldo] fp32 with
 * out[b, p * nc + c] = x[b, p, c0 + c] for p < HW, c < nc (the (h, w, c) flattening of a channel range; bf16 -> fp32 is exact) and
 * zeros in the columns HW * nc .. ldo - 1.  0 <= c0, c0 + nc <= C, HW * nc <= ldo.  Zero columns have zero mean and zero scatter, so
 * rows padded to a multiple of 64 go through tv_fid_accumulate and the caller trims the statistics to HW * nc. */
int tv_spatial_rows(const void* x, int B, int HW, int C, int ldc, int c0, int nc, float* out, int ldo, void* stream);
/* Streaming first and second moments of feature rows, fp64 on the device.
 * state: tv_fid_state_doubles(D) doubles (-1: D must be a multiple of 64 up to 8192), zero-initialised by the caller:
 * {count, unused, mean[D], M2[D * D]}, M2 the centred scatter matrix sum (x - mean)(x - mean)^T.  x [B, D] fp32 with row stride ldx;
 * n0 = the number of rows merged so far (the caller keeps it; state[0] mirrors it); scratch: B * D doubles.
 * The rows are merged one at a time, in order, by the pairwise (Chan) merge with a single sample (Welford's update), so the
 * state after N rows is the same bits however the rows were cut into calls, and independent of the launch geometry. */
long long tv_fid_state_doubles(int D);
int tv_fid_accumulate(const float* x, int B, int D, int ldx, long long n0, double* state, double* scratch, void* stream);

/* VF alignment term (R/transvae/losses/vae_loss.py:119-196): the DINOv2 ViT patch-feature extractor's own kernels and the loss
 * head (csrc/vf.hip; the plain LayerNorm is tv_rownorm_fwd mode 2 and tv_layernorm_rows, csrc/norm.hip) ---------------------
 * The ViT is facebookresearch/dinov2's DinoVisionTransformer (patch 14, LayerNorm eps 1e-6, LayerScale, erf-GELU MLP): patch
 * embedding, qkv / proj / fc1 / fc2 are tv_igemm_nt launches, the attention tv_attn_fwd (scale 1/8, no table).
 *
 * tv_vf_prep: fp32 NCHW images [B, 3, H, W] -> rows [B * gh * gw, 608] bf16, the 14 x 14 / stride-14 patches ((c, ky, kx) order,
 * 588 of 608 columns used, the rest zero) of the image resized bilinearly to (14 gh) x (14 gw) (align_corners=False, no
 * antialiasing; the interpolation weights are exact fractions rounded once) and, imagenet_norm != 0, normalised with the ImageNet
 * mean / std in fp32 before the one rounding to bf16. */
int tv_vf_prep(const float* img, void* rows, int B, int H, int W, int gh, int gw, int imagenet_norm, void* stream);
/* Token assembly: patch [B, n_patch, D] bf16, cls [D] fp32, pos [1 + n_patch, D] fp32 -> tok [B, 1 + n_patch, D] bf16;
 * row 0 = cls + pos[0], row 1 + p = patch[p] + pos[1 + p], one fp32 sum and one rounding each.  D % 8 == 0. */
int tv_vit_tokens(const void* patch, const float* cls, const float* pos, void* tok, int B, int n_patch, int D, void* stream);
/* LayerNorm with its affine on rows skip .. n_tok-1 of every image of x [B, n_tok, C] bf16 -> y [B, n_tok - skip, C] fp32
 * (two-pass statistics in registers, as tv_rownorm_fwd mode 2: y = (x - mean) rsqrt(var + eps_ln), affine-free, bf16). */
int tv_layernorm_rows(const void* x, const float* gamma, const float* beta, float* y, int B, int n_tok, int skip, int C, float eps,
                      void* stream);
/* VF head, fp32 throughout.  lat [B, D, Hl, Wl] fp32 is sampled bilinearly (align_corners=False) on the gh x gw grid of the
 * features feat [B * gh * gw, C] fp32 (token-major); y = w z + bias with w [C, D], bias [C] (both NULL: y = z, D == C <= 64;
 * with a projection D <= 32); per position cos = y . f / (max(|y|, 1e-12) max(|f|, 1e-12)); similarity = mean over all positions
 * (fp64 sum of tv_vf_head_partial_count(T) block partials, 8-byte aligned, in block order).
 * out[0] = max(margin - similarity, 0), out[1] = gate (1 when margin - similarity >= 0, else 0), out[2] = similarity.
 * dzr [T, D] receives d out[0] / d (sampled latent) WITHOUT the gate; zr [T, D] (the sampled latent) and ab [T, 2] are
 * written when given (both needed by tv_vf_head_dproj).
 * tv_vf_head_dproj: dw [C, D], db [C] = gate * gradient of out[0] w.r.t. the projection; gate = &out[1]; scratch of
 * tv_vf_head_dproj_partial_count(T, C, D) floats, slab partials added in slab order.
 * tv_bilinear_nchw_bwd: dlat [B, D, Hl, Wl] = gate[0] * (adjoint of the bilinear sampling applied to g [B, gh, gw, D]); gate may
 * be NULL (1).  Every element gathers its contributions in a fixed order: no atomics, the same bits on every run. */
long long tv_vf_head_partial_count(int T);
int tv_vf_head(const float* lat, const float* feat, const float* w, const float* bias, void* partials, float* out, float* dzr, float* zr,
               float* ab, int B, int D, int Hl, int Wl, int gh, int gw, int C, float margin, void* stream);
long long tv_vf_head_dproj_partial_count(int T, int C, int D);
int tv_vf_head_dproj(const float* feat, const float* zr, const float* ab, const float* w, const float* bias, const float* gate,
                     float* partials, float* dw, float* db, int T, int C, int D, void* stream);
int tv_bilinear_nchw_bwd(const float* g, const float* gate, float* dlat, int B, int D, int Hl, int Wl, int gh, int gw, void* stream);

/* Image pipeline (csrc/image.hip): decoded uint8 images in, uint8 grids out ------------------------------------------------------
 * tv_image_prep is torchvision's Resize(res) -> CenterCrop(res) -> ToTensor() as every script of the reference builds it
 * (R/train.py:141-144,396-399, R/evaluate.py:39-42, R/inference_example.py:13-16, P/generate_images.py:152-155; R/train_2.py:166-170
 * adds x*2-1) for a ragged batch in ONE launch, bit-equal to PIL's 8-bit bilinear resample: per axis a table of int32 fixed-point
 * coefficients (22 fraction bits, built on the host in float64 as PIL builds them), horizontal pass first, rounded and clipped to
 * uint8, then the vertical pass on those uint8 values; each pass is clip((2^21 + sum pixel * k) >> 22, 0, 255).  A pass whose
 * table index is negative is skipped (a copy; its output size must equal its input size), as PIL skips it.
 *   src       : device bytes holding the B images, RGB, HWC, uint8; src_bytes = its length
 *   desc_host / desc_dev : the same B descriptors on the host (checked here before the launch: extents, crop, tables -- the
 *               kernel indexes nothing that was not checked) and on the device (read by the kernel)
 *   coef_host / coef_dev : the coefficient tables, coef_len int32 each side.  A table for n output indices (n = res_w for the
 *               horizontal axis, res_h for the vertical one: only the rows / columns that survive the crop) with `ksize` taps at
 *               offset t is  first_tap[n], tap_count[n], k[n][ksize]  starting at coef[t]
 *   lut       : 256 device floats, the value of each byte: float(v) / 255.0f for ToTensor, that * 2 - 1 for the signed range
 *   out       : fp32 [B, 3, res_h, res_w], NCHW contiguous
 * Supported: any up-scale, down-scale ratios up to 16 per axis.  A larger ratio, a channel count other than 3 or an empty image
 * returns TV_ERR_UNSUPPORTED (with error text naming the image); other inconsistencies TV_ERR_ARG.  No device synchronisation. */
typedef struct tv_image_desc {
    long long offset;                     /* byte offset of pixel (0, 0) in src; any alignment */
    int in_h, in_w, row_stride, channels; /* row_stride in bytes, >= 3 * in_w; channels must be 3 */
    int out_h, out_w;                     /* size after the resize, before the crop */
    int crop_top, crop_left;              /* the output is rows crop_top .. crop_top + res_h - 1 of the resized image, likewise columns */
    int xtab, xk;                         /* horizontal table: offset into coef and taps per entry; xtab < 0: pass skipped */
    int ytab, yk;                         /* vertical table */
} tv_image_desc;
int tv_image_prep(const void* src, long long src_bytes, const tv_image_desc* desc_host, const tv_image_desc* desc_dev, int B,
                  const int* coef_host, const int* coef_dev, long long coef_len, const float* lut, float* out, int res_h, int res_w,
                  void* stream);
/* torchvision's make_grid(nrow, padding, pad_value) and save_image's quantisation in one launch (P/generate_images.py:181-235,
 * P/evaluate_transvae.py:227-249): img fp32 [B, 3, H, W] with element strides (sn, sc, sh, sw), read in place -> out uint8
 * [Hg, Wg, 3].  xmaps = min(nrow, B), ymaps = ceil(B / xmaps), Hg = (H + padding) ymaps + padding, Wg = (W + padding) xmaps + padding,
 * image k at ((k / xmaps)(H + padding) + padding, (k % xmaps)(W + padding) + padding), everything else pad_value; B == 1 gives the
 * image with no border (Hg = H, Wg = W).  Every value, pad_value included: x * 255, then + 0.5, each rounded to fp32 on its own,
 * clamp to [0, 255], truncate; NaN gives 0.  TV_IMAGE_SIGMOID applies a sigmoid to the pixels first (P/generate_images.py:106,139,163). */
#define TV_IMAGE_NONE 0
#define TV_IMAGE_SIGMOID 1
int tv_image_grid_u8(const float* img, long long sn, long long sc, long long sh, long long sw, void* out, int B, int H, int W, int nrow,
                     int padding, float pad_value, int transform, void* stream);

/* Latent-space statistics (csrc/latent.hip) ---------------------------------------------------------------------------------------
 * tv_latent_stats: streaming first and second moments of latents x [B, D, P] fp32 (positions contiguous; sn, sc = element strides of
 * the batch and channel axes, so a channel slice of a wider tensor is read in place), 1 <= D <= 64.  A sample is one (image,
 * position) pair.  state: 1 + D + D * D doubles, zero-initialised by the caller: {count, mean[D], M2[D * D]}, M2 the centred scatter
 * sum (x - mean)(x - mean)^T.  fp64 throughout: the batch mean per channel in a fixed order, the batch scatter about that mean, then
 * Chan's update.  scratch: 192 + min(256, ceil(B * P / 512)) * D * D doubles.  No atomics: the same sequence of calls gives the same
 * bits, and M2 is bit-symmetric; different cuts of one data set into calls agree to fp64 rounding, not bit for bit. */
int tv_latent_stats(const float* x, long long sn, long long sc, int B, int D, int P, double* state, double* scratch, void* stream);
/* Gaussian kernel density estimate in the log domain: out[i] = log sum_j exp(-inv_2h2 * |q_i - x_j|^2), i < M, j < N, fp32 in and
 * out; x [N, d] with row stride ldx, q [M, d] with row stride ldq, 1 <= d <= 64, N <= 2^30, inv_2h2 > 0 (= 1 / (2 h^2)).  The caller
 * adds the normaliser -log(N) - d/2 log(2 pi h^2) if it wants a density.  exclude_self != 0: q is x (M == N, N >= 2) and the term
 * j == i is dropped by index; duplicates of a point still count.  Squared distances are direct differences (an fmaf chain over k in
 * order), never the Gram form; a running reference (the nearest point so far) keeps every exponent <= 0, so a point far from all
 * others gets a finite value.  scratch: 128 * M doubles when M < 2048 (the data range is then cut into up to 64 slices whose
 * {reference, sum} pairs a second launch merges in order), unused otherwise (may be NULL).  The geometry is a function of (N, M, d)
 * alone; no atomics; bit-reproducible.  Rounding contract: DESIGN.md section 3.1 row T. */
int tv_kde_logdensity(const float* x, int N, const float* q, int M, int d, int ldx, int ldq, float inv_2h2, int exclude_self, float* out,
                      double* scratch, void* stream);

/* Linear probing of latents (csrc/probe.hip) ---------------------------------------------------------------------------------------
 * tv_probe_rows: fp32 latents x [B, D, h, w] (rows of w contiguous floats, planes of h * w; sn, sc = element strides of the batch
 * and channel axes, so the mu half of a moments tensor is read in place) -> bf16 rows [B, ld], the classifier's operand.  Every
 * channel is average-pooled to a gh x gw grid (gh | h, gw | w; gh = h, gw = w: no pooling) -- the fp32 sum of the window in scan
 * order times 1 / window --, standardised (v - mean[c]) * rstd[c] in fp32 and rounded once.  Column (py * gw + px) * D + c;
 * ld % 32 == 0 (tv_igemm_nt's c_in rule), ld >= gh * gw * D, the columns past gh * gw * D are exactly 0.  rows 16-byte aligned.
 * Rounding contract: DESIGN.md section 3.1 row C. */
int tv_probe_rows(const float* x, long long sn, long long sc, const float* mean, const float* rstd, void* rows, int B, int D, int h,
                  int w, int gh, int gw, int ld, void* stream);
/* Softmax cross-entropy of bf16 logits [B, ld] (columns 0 .. n_classes - 1 valid, ld % 8 == 0) against int64 labels [B] with label
 * smoothing: per row lse - (1 - eps) x_y - (eps / n) sum_j x_j, and the rank of the label's logit = the columns with a strictly
 * greater logit plus the columns with an equal logit and a lower index.  dlogits (bf16 [B, ld]; NULL: evaluation) receives
 * grad_scale * (softmax - target), target = (1 - eps) [j == y] + eps / n, computed in fp32 and rounded once, pad columns exactly 0.
 * state: 4 doubles {loss sum, rows counted, top-1 hits (rank 0), top-5 hits (rank < 5)} that the call ADDS to (zero it to start; read it
 * with one synchronisation when the metrics are wanted).  A row whose label is outside [0, n_classes) gets a zero gradient row and is not counted.
 * partials: tv_softmax_xent_partial_count(B) doubles of scratch.  One wave per row, the row in registers up to n_classes = 4096,
 * three sweeps over memory above; block partials are added in block order in fp64: no atomics, bit-reproducible.
 * Rounding contract: DESIGN.md section 3.1 row C. */
long long tv_softmax_xent_partial_count(int B);
int tv_softmax_xent(const void* logits, const long long* labels, void* dlogits, double* state, double* partials, int B, int n_classes,
                    int ld, float label_smoothing, float grad_scale, void* stream);

/* Latent DiT: adaLN-Zero conditioning and the flow-matching edge (csrc/dit.hip) --------------------------------------------------------
 * Token matrices are bf16 [B N, C] (row r belongs to sample r / N; C % 8 == 0; 16-byte aligned).  mod is the fp32 [B, ld] modulation
 * matrix of the block; shift / scale / gate are C columns of it starting at the given offsets (offset + C <= ld).  dmod has mod's
 * shape; the backward calls WRITE their column ranges of it (no accumulation, no atomics: per lane the rows in order, per block the
 * waves in order, then the row slabs of a sample in order -- the same bits on every run).  Rounding contract: DESIGN.md section 3.1
 * row E; protocol: section 3.4.
 * tv_adaln_fwd: y = bf16(fma(xhat, 1 + scale, shift)), xhat = (x - mean) rstd with two-pass fp32 statistics of the row (the scheme
 * of tv_rownorm_fwd mode 2), affine-free.  C <= 1536.
 * tv_adaln_bwd: statistics recomputed; g = dy (1 + scale); dx = bf16(rstd (g - mean(g) - xhat mean(g xhat)) + dres) (dres bf16 or
 * NULL, joined in fp32); dmod[b, shift_off + c] = sum_n dy, dmod[b, scale_off + c] = sum_n dy xhat.  The two ranges must not overlap.
 * partials: tv_adaln_bwd_partial_count(B, N, C) floats of scratch. */
int tv_adaln_fwd(const void* x, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C, float eps, void* stream);
long long tv_adaln_bwd_partial_count(int B, int N, int C);
int tv_adaln_bwd(const void* x, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres, void* dx, float* dmod,
                 float* partials, int B, int N, int C, float eps, void* stream);
/* tv_gate_residual_fwd: out = bf16(fma(gate, y, x)).  tv_gate_residual_bwd: dy = bf16(gate dout), dmod[b, gate_off + c] = sum_n dout y;
 * the gradient of x is dout itself.  C <= 2048.  partials: tv_gate_residual_bwd_partial_count(B, N, C) floats of scratch. */
int tv_gate_residual_fwd(const void* x, const void* y, const float* mod, int gate_off, int ld, void* out, int B, int N, int C, void* stream);
long long tv_gate_residual_bwd_partial_count(int B, int N, int C);
int tv_gate_residual_bwd(const void* dout, const void* y, const float* mod, int gate_off, int ld, void* dy, float* dmod, float* partials, int B,
                         int N, int C, void* stream);
/* Flow matching on fp32 latents lat [B, D, h, w] (sn, sc = element strides of the batch and channel axes, as tv_probe_rows takes
 * them).  With x = (lat - mean[c]) * rstd[c] (two fp32 roundings) and patch size p (p | h, p | w), token (ty, tx) of sample b is row
 * b N + ty (w / p) + tx, N = (h / p)(w / p), and element (py, px, c) of its patch is column (py p + px) D + c; ld % 32 == 0,
 * ld >= p p D, the columns past p p D are exactly 0.  noise is dense fp32 [B, D, h, w], t fp32 [B].
 * tv_flow_rows: rows = bf16(fma(t, x, (1 - t) e)); noise NULL: rows = bf16(x), the plain patchify (t is not read).
 * tv_flow_loss: d = pred - (x - e) over the real columns; out[0] = sum d^2, out[1] = out[0] / (B N p p D), fp64 (per thread in
 * element order, per wave a butterfly, per block its four waves in order, then the blocks in order); dpred (bf16 or NULL) =
 * bf16(fp32(2 grad_scale / count) * d), pad columns exactly 0.  partials: tv_flow_loss_partial_count(...) doubles of scratch.
 * tv_flow_euler: x (dense fp32 [B, D, h, w]) += dt v with v read from bf16 rows [B N, ld]; guided != 0: v has 2 B N rows, the first
 * B N conditional (v_c), the rest unconditional (v_u), and v = fma(cfg_scale, v_c - v_u, v_u); every sum is one fp32 operation. */
int tv_flow_rows(const float* lat, long long sn, long long sc, const float* mean, const float* rstd, const float* noise, const float* t, void* rows,
                 int B, int D, int h, int w, int patch, int ld, void* stream);
long long tv_flow_loss_partial_count(int B, int D, int h, int w, int patch, int ld);
int tv_flow_loss(const void* pred, const float* lat, long long sn, long long sc, const float* mean, const float* rstd, const float* noise,
                 void* dpred, double* out, double* partials, int B, int D, int h, int w, int patch, int ld, float grad_scale, void* stream);
int tv_flow_euler(float* x, const void* v, int B, int D, int h, int w, int patch, int ld, float dt, float cfg_scale, int guided, void* stream);
/* tv_flow_loss_cos: tv_flow_loss with a cosine term per position (latent pixel): the D columns q D .. q D + D - 1 of a row, q < p p, any
 * D.  With v = x - e as above and the fp32 fma chains np2 = sum p^2, nv2 = sum v^2, dot = sum p v over c = 0 .. D - 1, eps = 1e-8:
 * cos = fp32(dot / sqrt(np2 max(nv2, eps^2))), formed in fp64 and rounded once; np2 <= eps^2: cos = 0 and the term gives no gradient
 * (unlike autograd through cosine_similarity, which returns v / (|v| eps) for a zero prediction).  out = 5 doubles {sum d^2, its
 * mean (the bits of tv_flow_loss), sum (1 - cos), its mean over the B h w positions, mse mean + cos_weight cos mean}, every sum
 * in the order of tv_flow_loss.  dpred (bf16 or NULL) = bf16(fma(-fp32(grad_scale cos_weight / (B h w)), gc, fp32(2 grad_scale /
 * count) d)), gc = (v rv - (cos p) rp) rp with rp = fp32(1 / sqrt(np2)), rv = fp32(1 / sqrt(max(nv2, eps^2))): formed in fp32, rounded
 * once, pad columns exactly 0.  cos_weight >= 0.  partials: tv_flow_loss_cos_partial_count(...) doubles of scratch.
 * tv_flow_heun: x holds the predictor's result x + dt g1; x = fma(dt / 2, g2 - g1, x).  g_k is read from v_k (bf16 rows, B N of them, or
 * 2 B N with guided_k != 0) as tv_flow_euler reads its velocity: fma(cfg_scale, v_c - v_u, v_u) if guided_k, the conditional rows
 * otherwise.  The two flags are independent.  Rounding contract: DESIGN.md section 3.1 row E (its last line); protocol: section 3.7. */
long long tv_flow_loss_cos_partial_count(int B, int D, int h, int w, int patch, int ld);
int tv_flow_loss_cos(const void* pred, const float* lat, long long sn, long long sc, const float* mean, const float* rstd, const float* noise,
                     void* dpred, double* out, double* partials, int B, int D, int h, int w, int patch, int ld, float cos_weight, float grad_scale,
                     void* stream);
int tv_flow_heun(float* x, const void* v1, const void* v2, int B, int D, int h, int w, int patch, int ld, float dt, float cfg_scale, int guided1,
                 int guided2, void* stream);

/* LightningDiT block variants: RMSNorm adaLN (csrc/dit.hip), per-head qk-norm with RoPE (csrc/qk_norm.hip), SwiGLU (csrc/lightning.hip) ---
 * The conventions of the DiT block above: bf16 token matrices [B N, C], 16-byte aligned, C % 8 == 0; the fp32 [B, ld] modulation
 * matrix read by column offsets; every sum that crosses rows goes through scratch partials in a fixed order and is WRITTEN (no
 * accumulation, no atomics anywhere in the file: the same bits on every run).  Rounding contract: DESIGN.md section 3.1 row J;
 * protocol: section 3.6.
 * tv_adaln_rms_fwd: xhat = x rsqrt(mean(x^2) + eps) (one fp32 chain per lane, a butterfly; no mean), z = xhat w rounded once (w fp32
 * [C]), y = bf16(fma(z, 1 + scale, shift)).  One wave per row, C <= 1536.
 * tv_adaln_rms_bwd: the statistic recomputed; g = dy ((1 + scale) w); dx = bf16(rstd (g - xhat mean(g xhat)) + dres) (dres bf16 or
 * NULL, joined in fp32); dmod[b, shift_off + c] = sum_n dy; with S[b, c] = sum_n dy xhat (per wave its 16 rows of a 64-row slab,
 * the four waves, the slabs of a sample, all in order): dmod[b, scale_off + c] = w[c] S[b, c] and dw[c] = sum_b fma(1 + scale[b, c],
 * S[b, c], .) (sample b in lane b % 16 in order, the sixteen lanes in order), fp32 [C], written.  The two ranges must not overlap.
 * partials: tv_adaln_rms_bwd_partial_count(B, N, C) floats of scratch. */
int tv_adaln_rms_fwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, void* y, int B, int N, int C, float eps,
                     void* stream);
long long tv_adaln_rms_bwd_partial_count(int B, int N, int C);
int tv_adaln_rms_bwd(const void* x, const float* w, const float* mod, int shift_off, int scale_off, int ld, const void* dy, const void* dres, void* dx,
                     float* dmod, float* dw, float* partials, int B, int N, int C, float eps, void* stream);
/* Per-head RMSNorm of q and k, then the RoPE of tv_rope_qk (csrc/qk_norm.hip, the <64> kernels), on qkv [B, N, 3, heads, 64] bf16;
 * wq, wk fp32 [64]; rope_tab [N, 4, 32] fp32 or NULL (no rotation).
 * tv_qknorm_rope_fwd: per (token, head), q and k alike: r = rsqrt(mean_64(q^2) + eps) (eight lanes of 16 bytes, a three-step
 * butterfly), z = (q r) w, rotated in fp32 (two products and their sum per output, as tv_rope_qk), rounded to bf16 once; the v third
 * is copied bit for bit.  out may be qkv itself (each 64-vector is read whole before it is written) or must not overlap it.
 * tv_qknorm_rope_bwd: qkv holds the RAW projections, dqkv the gradient from tv_attn_bwd called WITH the table (so dq / dk are
 * gradients of the un-rotated z).  In place on dqkv: g = dq wq, qh = q r, dq_raw = bf16(r fma(-qh, mean_64(g qh), g)); k likewise; v
 * untouched.  dwq[j] = sum over (b, n, head) of dq_j qh_j and dwk likewise, fp32 [64], written: per lane group its vectors in pass
 * order, the 32 groups of a block in order, block k in lane k % 64 in order, the 64 lanes in order.  A zero head vector gives
 * exactly 0 forward and a finite gradient.  partials: tv_qknorm_rope_bwd_partial_count(B, N, heads) floats of scratch. */
int tv_qknorm_rope_fwd(const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads, float eps,
                       void* stream);
long long tv_qknorm_rope_bwd_partial_count(int B, int N, int heads);
int tv_qknorm_rope_bwd(const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N, int heads,
                       float eps, void* stream);
/* SwiGLU on u bf16 [T, 2 Hp] = [x1 | x2], Hp % 32 == 0: h [T, Hp] = bf16((x1 s) x2), s = 1 / (1 + expf(-x1)) with the IEEE division.
 * tv_swiglu_bwd: du [T, 2 Hp] = [bf16((dh x2) (s fma(x1, 1 - s, 1))) | bf16(dh (x1 s))].  Finite for every finite bf16 x1 (at
 * x1 = -3e38: silu = -0, derivative -0; at +3e38: silu = x1, derivative 1); x1 = 0 gives exactly 0. */
int tv_swiglu_fwd(const void* u, void* h, long long T, int Hp, void* stream);
int tv_swiglu_bwd(const void* u, const void* dh, void* du, long long T, int Hp, void* stream);

/* The head_dim 72 family (csrc/attention_hd.hip; the qk-norm pair is csrc/qk_norm.hip, one template over head_dim with the entries
 * above; DiT-XL / LightningDiT-XL: 1152 = 16 heads of 72) -----------------------------------------------------------------------------
 * The entries above at another head dimension: the same argument lists plus `head_dim`, which must be 72 here (any other value
 * returns TV_ERR_ARG with an error text naming head_dim; 64 has the entries above).  Heads sit at their natural stride, nothing in
 * HBM is padded: qkv [B, N, 3, heads, 72] bf16 (a head vector is 144 bytes = nine 16-byte pieces), o [B, N, heads, 72] bf16, lse
 * [B, heads, N] fp32, delta [2, B, heads, N] fp32 scratch, the table [N, 4, 36] fp32 (cos1, sin1, cos2, sin2 of 36 pairs), wq / wk
 * / dwq / dwk fp32 [72].  Tensors 16-byte aligned; B N 3 heads < 2^31.  The pads of the MFMA shapes (72 -> 80 in q.k, -> 96 in P V)
 * live in registers and LDS only and are zeros by construction: no load or store touches an address outside the head vector, token
 * row or statistics row it belongs to.  No atomics; the same bits on every run.
 * tv_attn_fwd_hd / tv_attn_bwd_hd: as tv_attn_fwd / tv_attn_bwd, any N >= 1; the policies are stated in the file header.
 * tv_rope_qk_hd: as tv_rope_qk.
 * tv_qknorm_rope_fwd_hd / _bwd_hd: as tv_qknorm_rope_fwd / _bwd with r = rsqrt(mean_72(q^2) + eps): a head vector is a 16-lane group,
 * lanes 0..8 one piece each (a chain of 8 FMAs), lanes 9..15 zeros that touch no memory, a four-step xor butterfly; mean = sum times
 * fp32(1 / 72).  dwq / dwk: per lane group its vectors in pass order, the 16 groups of a block in order, block k in lane k % 64 in
 * order, the 64 lanes in order.  partials: tv_qknorm_rope_bwd_hd_partial_count(B, N, heads, head_dim) floats (-1: bad arguments).
 * Rounding contract: DESIGN.md section 3.1 row Y. */
int tv_attn_fwd_hd(const void* qkv, void* o, float* lse, int B, int N, int heads, int head_dim, float scale, void* stream);
int tv_attn_bwd_hd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, const float* rope_tab, void* dqkv, int B,
                   int N, int heads, int head_dim, float scale, void* stream);
int tv_rope_qk_hd(void* qkv, const float* tab, int B, int N, int heads, int head_dim, int transpose, void* stream);
int tv_qknorm_rope_fwd_hd(const void* qkv, const float* wq, const float* wk, const float* rope_tab, void* out, int B, int N, int heads,
                          int head_dim, float eps, void* stream);
long long tv_qknorm_rope_bwd_hd_partial_count(int B, int N, int heads, int head_dim);
int tv_qknorm_rope_bwd_hd(const void* qkv, const float* wq, const float* wk, void* dqkv, float* dwq, float* dwk, float* partials, int B, int N,
                          int heads, int head_dim, float eps, void* stream);


/* Generation metrics (csrc/genmetrics.hip) -------------------------------------------------------------------------------------------
 * Squared distance of the two pairwise kernels: D(a, b) = sum_c (a_c - b_c)^2 as ONE fp32 chain over c = 0 .. d - 1 in order, diff =
 * a_c - b_c rounded once, acc = fmaf(diff, diff, acc); no partial chains (the accumulator stays in a register across the d-chunks),
 * never the Gram form.  D(a, b) and D(b, a) are the same bits, and the bits of a pair depend on nothing but the two rows and d.
 * Bound against fp64: (d + 2) u D, u = 2^-24.  1 <= d <= 8192, fp32 rows with strides ldx, ldq >= d; float4 loads when the bases are
 * 16-byte aligned and the strides multiples of 4, scalar loads otherwise (the same bits).
 * tv_knn_radius: for the queries i = i0 .. i0 + M - 1 of x [N, d], r2[i - i0] = the k-th smallest D(x_i, x_j) over j != i; self is
 * excluded by index, duplicates of a point still count (= the (k + 1)-th smallest with self included).  1 <= k <= 8, N >= k + 1.
 * tv_manifold_hits: hit[i] (int32) = 1 when some j < N has D(q_i, x_j) <= r2[j], compared on the fp32 values, else 0; i < M.
 * scratch: when ceil(M / 64) < 512 the data range may be cut into up to 32 slices that a second launch merges in slice order:
 * 256 * M floats (tv_knn_radius) or 32 * M ints (tv_manifold_hits); unused and may be NULL otherwise.  The geometry is a function of
 * (N, M) alone, there are no atomics, and the output does not depend on the geometry: bit-reproducible, and the same for every cut of
 * the query range into calls.  Every coordinate and every r2 must be finite: the k-lists are kept with fminf / fmaxf, which drop a NaN
 * distance and repeat a list entry in its place, so non-finite rows corrupt the radii without a sign of it (evaluate_dit checks its
 * features; a direct caller checks its own).  Rounding contract: DESIGN.md section 3.1 row S; protocol: section 3.5. */
int tv_knn_radius(const float* x, int N, int d, int ldx, int i0, int M, int k, float* r2, float* scratch, void* stream);
int tv_manifold_hits(const float* q, int M, int ldq, const float* x, int N, int ldx, const float* r2, int d, int* hit, int* scratch,
                     void* stream);
/* Ball counts (density / coverage, Naeem et al. 2020) on the same distance chain and the same `<=` on the fp32 values:
 *   radius_of = 0: count[i] = #{j < N : D(q_i, x_j) <= r2[j]}, r2 [N], one squared radius per data point;
 *   radius_of = 1: count[i] = #{j < N : D(q_i, x_j) <= r2[i]}, r2 [M], one squared radius per query.
 * count int32 [M].  scratch: 32 * M ints under the rule of tv_manifold_hits; the slices are added by the merge launch (integers: no
 * order question).  count[i] > 0 at radius_of = 0 is tv_manifold_hits' hit[i]. */
int tv_ball_counts(const float* q, int M, int ldq, const float* x, int N, int ldx, const float* r2, int d, int radius_of, int* count,
                   int* scratch, void* stream);
/* Polynomial-kernel sums (KID): for every subset s < S, sums[s] = sum over 0 <= i, j < m of k(a[ia[s m + i]], b[ib[s m + j]]), the
 * pairs with i == j left out when skip_equal_position != 0.  a, b: fp32 rows with strides lda, ldb >= d; ia, ib: int32 [S, m] row
 * indices, which the CALLER keeps inside a and b (they are read on the device and cannot be checked here).  Nothing is gathered and
 * no m x m matrix is formed; one launch covers all subsets, 64 x 64 pairs per block through the staging of the pairwise kernels.
 * k(x, y): dot = ONE fp32 chain over c = 0 .. d - 1 in order, dot = fmaf(x_c, y_c, dot), the accumulator in a register across the
 * d-chunks; then fp64 without contraction, t = (double)dot * gamma + coef0, k = (t * t) * t.  A thread adds its pairs in a fixed
 * order, a block its threads in thread order, a second launch the blocks of a subset in block order: no atomics, the same bits on
 * every run and for float4 and scalar loads.  scratch: tv_poly_kernel_scratch_doubles(m, S) doubles (-1: 1 <= m <= 2^16,
 * 1 <= S <= 65535).  Bound against fp64 per sum: sum_pairs 3 t^2 gamma (d + 2) u sum_c |x_c y_c|. */
long long tv_poly_kernel_scratch_doubles(int m, int S);
int tv_poly_kernel_sums(const float* a, int lda, const int* ia, const float* b, int ldb, const int* ib, int m, int S, int d, double gamma,
                        double coef0, int skip_equal_position, double* sums, double* scratch, void* stream);
/* Softmax statistics of fp32 logits [B, K] (row stride ld >= K, 1 <= K <= 4096) for the Inception Score.  state: 2 + K doubles
 * {rows, sum_rows sum_k p log p, sum_rows p_k} that the call ADDS to (zero it to start).  Everything after the load is fp64: z - max,
 * exp, the row sum s in k order, log, p = e / s, log p = (z - max) - log s, the row's sum of p log p in k order.  The rows are added
 * to the state one at a time in row order, so the state after n rows has the same bits however the rows were cut into calls.
 * scratch: B * (K + 1) doubles.  Bound per state entry: 16 K 2^-53 relative to the sum of the absolute terms. */
int tv_softmax_stats(const float* logits, int B, int K, int ld, double* state, double* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSVAE_HIP_H */
