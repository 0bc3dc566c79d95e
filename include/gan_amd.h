/* gan_amd.h — C ABI of the MI355X (gfx950) Pix2Pix / CycleGAN training hot path.
 *
 * The reference (kingjosephm/GAN) has no FFI / plugin interface: its hot path is Python calling
 * tf.keras layers.  Each entry point below replaces one Keras layer invocation
 * (or its autodiff counterpart) that the reference instantiates; the reference file:line it
 * replaces is cited per function.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *  - plain C, raw device pointers, POD structs; no torch / hip types in signatures
 *    (gan_stream_t is a hipStream_t passed as void*).
 *  - every call only ENQUEUES work on `stream` (hipGraph-capturable, no allocation, no sync).
 *  - return: 0 ok; <0 invalid argument / unsupported shape (GAN_E_*); >0 a hipError_t.
 *  - activations NHWC; a GanTensor may be a channel slice of a wider buffer (pitch > c), which is
 *    how skip-concat (base_gan.py:206,221) and the discriminator input concat (base_gan.py:139)
 *    are realised without a copy.
 *  - dtype GAN_F32: fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) — the parity path.
 *    dtype GAN_BF16: bf16 storage, v_mfma_f32_16x16x32_bf16, fp32 accumulate — the fast path.
 *    dtype GAN_F16: fp16 storage, v_mfma_f32_16x16x32_f16, fp32 accumulate and fp32 master weights; used with the
 *    dynamic loss scale below (BASELINE.json config 5; the reference itself has no mixed precision).
 *  - every descriptor struct starts with `uint32_t struct_size` = sizeof(the struct) as the CALLER compiled it; an entry
 *    point returns GAN_E_ARG when it differs from the library's own sizeof (descriptors grow by appending fields).
 *  - convolution weights are consumed in "NK" layout [16 taps][rows][k] (k contiguous), produced
 *    from the fp32 Keras-layout master by gan_weights_prepare().
 */
#ifndef GAN_AMD_H
#define GAN_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* gan_stream_t;

enum { GAN_F32 = 0, GAN_BF16 = 1, GAN_F16 = 2 };
enum { GAN_ACT_NONE = 0, GAN_ACT_LRELU = 1, GAN_ACT_RELU = 2, GAN_ACT_TANH = 3 };
enum { GAN_E_ARG = -1, GAN_E_SHAPE = -2, GAN_E_WORKSPACE = -3 };

typedef struct GanTensor {
  void* ptr;          /* element (n=0,h=0,w=0,channel 0 of this view) */
  int32_t n, h, w, c; /* c: channels the op touches */
  int32_t pitch;      /* elements between consecutive pixels (>= c) */
} GanTensor;

/* ---- convolutions ------------------------------------------------------------------------- */
/* Optional fused backward epilogue of the two dgrad entry points: the backward of the layer BELOW (its
 * normalisation + activation, base_gan.py:83-87 / :113-120 under tf.GradientTape) starts in the epilogue of the
 * launch that produces the gradient w.r.t. that layer's activation.  For the first `cols` channels of y the stored
 * value is not da but
 *     dz = (da + add) * act'(z) * 2*dropmask,   z = gamma*(ref - mean)*rstd + beta      (mean != NULL; ref = that layer's y)
 *     dz = (da + add) * act'(ref)                                                       (mean == NULL; ref = saved activation)
 * and, with mean != NULL, per-tile partial sums (sum dz, sum dz*xhat) are written to GanConvDesc.stats_partial as
 * [group][chunk][cols][2] (groups = GanConvDesc.stats_groups); gan_norm_act_bwd_fused() finishes the layer.  Channels
 * >= cols (the skip half of a decoder concat) are stored unchanged.  Honoured only when gan_conv_plan_info()[4] > 0. */
typedef struct GanBwdFuse {
  GanTensor ref;             /* y (pre-normalisation) or the saved activation a; same n, h, w as GanConvDesc.y */
  GanTensor add;             /* optional second upstream gradient (skip connection); ptr NULL = none */
  const float* mean;         /* [groups][cols]; NULL = activation-only backward */
  const float* rstd;
  const float* gamma;        /* [cols] */
  const float* beta;
  const uint8_t* dropmask;   /* optional dense 0/1 bytes [n][h][w][mask_pitch] */
  int32_t mask_pitch;
  int32_t act;               /* GAN_ACT_LRELU | GAN_ACT_RELU */
  float slope;
  int32_t cols;              /* multiple of 8 */
} GanBwdFuse;

/* Optional: a split-K launch of a SMALL layer finishes the whole layer in its slab-reduce kernel (one launch instead of
 * reduce + statistics finalize + apply): a workgroup owns 8 channels of all rows of a statistics group (at most 1024 rows), so
 * it sums the K slabs, takes the statistics and applies them without leaving the kernel.
 * Forward entry points (with GanConvDesc.stats_groups): y = conv output as usual, out = act(dropout(gamma*(y-mean)*rstd+beta))
 * (Conv -> BN|IN -> [Dropout] -> act of base_gan.py:77-87, :106-120); mean / rstd / moving averages are written as
 * gan_norm_stats would.  dgrad entry points (with GanConvDesc.bwd_fuse, which names the layer below): out = dy of that layer,
 * dgamma / dbeta accumulated; the first bwd_fuse->cols channels of GanConvDesc.y are then NOT written (dz stays in registers;
 * channels >= cols receive the plain gradient as usual).
 * Honoured only when gan_conv_plan_info()[4] == -1: the caller asks first and passes norm_fuse = NULL otherwise - a launch
 * whose plan cannot honour a non-NULL norm_fuse returns GAN_E_SHAPE (the caller would have dropped the layer's own
 * normalisation launches on the strength of the query). */
typedef struct GanNormFuse {
  GanTensor out;
  const float* gamma;
  const float* beta;
  float* mean;               /* forward: [groups][c] written */
  float* rstd;
  float* moving_mean;        /* forward, optional */
  float* moving_var;
  float eps, momentum;
  const uint8_t* dropmask;   /* forward, optional: dense 0/1 bytes [n][h][w][c] */
  int32_t act;
  float slope;
  float* dgamma;             /* backward, optional */
  float* dbeta;
  int32_t accumulate;
} GanNormFuse;

typedef struct GanConvDesc {
  uint32_t struct_size;  /* sizeof(GanConvDesc) of the caller's build */
  int32_t dtype;
  int32_t stride;        /* Conv2D: 1 or 2 (k4, zero pad 1 each side); Conv2DTranspose: 2 */
  GanTensor x;           /* GEMM-K side tensor; x.c must be a multiple of 8 (zero-padded channels) */
  GanTensor y;           /* produced tensor; y.c = channels written (pitch may be larger) */
  const void* w;         /* NK weights [16][w_rows][x.c], dtype */
  int32_t w_rows;        /* >= y.c */
  const float* bias;     /* optional [y.c] */
  int32_t act;           /* epilogue activation (GAN_ACT_*) applied after bias */
  float slope;           /* LeakyReLU alpha */
  int32_t y_f32;         /* 1: write y as fp32 whatever dtype is (used for logits) */
  void* workspace;       /* split-K slabs; size from gan_conv_workspace_bytes() */
  size_t workspace_bytes;
  float* stats_partial;  /* optional: fused normalisation statistics — per-tile (sum, sum^2) partials of y,   */
  int32_t stats_groups;  /* laid out [group][chunk][y.c][2]; emitted only if gan_conv_plan_info()[4] > 0     */
  size_t stats_partial_bytes; /* size of that region: groups * chunks * channels * 8 bytes are written (GAN_E_WORKSPACE if short) */
  const GanBwdFuse* bwd_fuse; /* optional (dgrad entry points only), see above */
  const GanNormFuse* norm_fuse; /* optional, see above */
} GanConvDesc;

/* Conv2D(k4, strides=s, no bias | bias) — base_gan.py:77-79 ('same', s=2), :145-148 and :157-161
 * (ZeroPadding2D + 'valid', s=1).  w = prepared from HWIO master with gan_weights_prepare(transposed). */
int gan_conv2d_fwd(const GanConvDesc* d, gan_stream_t stream);
/* Gradient of the above w.r.t. its input (tf.GradientTape, pix2pix.py:210-211): x := dy, y := dx,
 * w = native NK copy of the HWIO master ([tap][cin][cout]). */
int gan_conv2d_dgrad(const GanConvDesc* d, gan_stream_t stream);
/* Conv2DTranspose(k4, strides=2, 'same') — base_gan.py:106-110, :201-204 (bias + tanh head).
 * w = native NK copy of the (kh,kw,cout,cin) master. */
int gan_convT2d_fwd(const GanConvDesc* d, gan_stream_t stream);
/* Gradient of Conv2DTranspose w.r.t. its input: x := dy (2h x 2w), y := dx (h x w),
 * w = transposed NK copy ([tap][cin][cout]). */
int gan_convT2d_dgrad(const GanConvDesc* d, gan_stream_t stream);
size_t gan_conv_workspace_bytes(const GanConvDesc* d, int op /*0 conv_fwd,1 conv_dgrad,2 convT_fwd,3 convT_dgrad*/);
/* launch plan the library picks for this problem: info[5] = {BM, BN, splitK, parities, fused-stats chunks per group}
 * (BM = 0: streaming kernel family BN = 1 | 2, or BN = 8: the column-owner kernel - one launch, 8 output channels of every row per
 * workgroup, only with norm_fuse; BM = 1024: parity-patch kernel; info[4] = -1: norm_fuse is honoured, the launch finishes the layer) */
int gan_conv_plan_info(const GanConvDesc* d, int op, int32_t* info);
/* Which main loop a 256-row tile of this launch takes: 0 = one staged A tile per tap (conv_gemm_pp_kernel), 2 | 4 = the taps of a
 * kernel row that read the same pixels one grid column apart share one staged A tile (conv_gemm_ps_kernel; option conv.tap_share).
 * 0 for every other tile; < 0: error code.  Results of the two loops differ in fp32 summation order only. */
int gan_conv_tap_shared(const GanConvDesc* d, int op);

/* ---- layer stack: a run of consecutive small split-K layers in ONE launch -------------------------------------------------
 * The inner layers of the U-Net (base_gan.py:183-193: down5..down8, up1..up3 at batch 16; most of the generator at the reference's
 * CycleGAN batch of 1) are latency chains: a GEMM into fp32 slabs plus the slab reduce that finishes the layer (GanNormFuse), each a
 * few microseconds of work behind a launch.  gan_conv_stack_* runs such a run of layers from ONE persistent kernel: a resident grid
 * walks the layers, a grid barrier separates the phases, and what crosses workgroups inside the launch is written through / read
 * around the per-XCD L2s.  Eligible: a launch whose gan_conv_plan_info()[4] == -1 (norm_fuse honoured), tile 64x128 or 16x128, at
 * most 512 rows per statistics group; layer i+1 must consume what layer i produced (the caller's op order), all one dtype.
 *   plan   : host side, once per run of layers -> an opaque blob (gan_conv_stack_plan_bytes(n) bytes) that the caller ALSO copies
 *            into device memory (256-byte aligned) - the library allocates nothing;
 *   launch : enqueue-only (hipGraph-capturable).  barrier_state: gan_conv_stack_barrier_bytes() of ZEROED device memory, 128-byte
 *            aligned, owned by this plan for good (monotonic counters); err_flag: device int32, set to 1 if a grid barrier timed out
 *            (~2 s: the grid could not become resident) - results are then undefined, the kernel still terminates.
 * Measured (round 4, tools/bench_stack.py, hipGraph replay on one stream): 5 layers at Pix2Pix batch 16 89.6 us as a stack against
 * 79.3 us as ten launches; 9 layers at CycleGAN batch 1 141 against 122 us - two grid barriers (2.2 us each + the drain of the
 * write-through stores) cost more than the two kernel boundaries of a replayed graph (~1.5 us each), and every layer keeps its four
 * dependent global round trips.  The in-tree callers therefore use it only on request (option conv.stack).
 * At most TWO stack launches may run concurrently on one GPU (two workgroups of it fit on every CU; a third resident grid could
 * wait for CUs the other two hold while they wait for each other). */
int gan_conv_stack_eligible(const GanConvDesc* d, int op);   /* 1: this launch can be a layer of a stack, 0: not, < 0: error code */
size_t gan_conv_stack_plan_bytes(int32_t n);
int gan_conv_stack_plan(const GanConvDesc* const* descs, const int32_t* ops /* as gan_conv_plan_info's op */, int32_t n, void* host_plan,
                        size_t plan_bytes);
int gan_conv_stack_launch(const void* host_plan, const void* dev_plan, void* barrier_state, int32_t* err_flag, gan_stream_t stream);
size_t gan_conv_stack_barrier_bytes(void);

/* Optional: the wgrad launch itself applies the optimiser step (TF-form Adam, base_gan.py:247-252 / pix2pix.py:213-216) to the
 * kernel it has just differentiated and refreshes its typed NK copies - the fp32 gradient is then neither written nor read back
 * (dw stays untouched).  Bit-identical to gan_conv_wgrad followed by gan_adam_prepare_multi.  gan_adam_begin must have run for
 * this step (lr_t).  Not for fp16 steps with dynamic loss scaling (their update waits for the whole-step inf/nan check and
 * un-scales).  Two carriers: the epilogue of an un-split launch of the 128x128 LDS-DMA kernel, and - for every launch that
 * splits its reduction, the ping-pong kernel included - the slab-reduce kernel, which then ends in the optimiser step instead of
 * writing the fp32 gradient (option wgrad.reduce_adam, default 1; kernels of at least
 * wgrad.reduce_adam_min_params parameters).  Honoured only when gan_wgrad_adam_fused() returns 1 for the
 * descriptor (16-bit storage, accumulate == 0, channel counts multiples of 8, no tap folding); the caller asks first and passes adam_fuse = NULL
 * otherwise - gan_conv_wgrad returns GAN_E_SHAPE for a non-NULL adam_fuse its plan cannot honour. */
typedef struct GanAdamFuse {
  float* master;             /* fp32 [16][big_c][small_c]: the layout of dw */
  float* m;
  float* v;
  void* nk_native;           /* [16][big_c][small_c] dtype, or NULL */
  void* nk_transposed;       /* [16][small_c][big_c] dtype, or NULL */
  const float* lr_t;         /* device scalar written by gan_adam_begin */
  float beta1, beta2, eps;
} GanAdamFuse;

typedef struct GanWgradDesc {
  uint32_t struct_size;  /* sizeof(GanWgradDesc) of the caller's build */
  int32_t dtype;
  int32_t stride;        /* 1 or 2 */
  GanTensor big;         /* tensor on the fine grid  (Conv2D: layer input x;  Conv2DTranspose: dy) */
  GanTensor small;       /* tensor on the coarse grid (Conv2D: dy;            Conv2DTranspose: layer input x) */
  float* dw;             /* fp32 [16][big_c][small_c]: HWIO for Conv2D, (kh,kw,cout,cin) for Conv2DTranspose; 16-byte aligned */
  int32_t big_c, small_c;/* real channel counts written (<= big.c, small.c which are 8-padded) */
  int32_t accumulate;    /* 1: dw += result (a net called several times per step, cycle_gan.py:252-255) */
  void* workspace;
  size_t workspace_bytes;
  int32_t concurrent;    /* scheduling hint: nonzero = this launch shares the GPU with other streams' kernels (a side lane of a
                            captured step): the planner then prefers fewer, longer blocks (less slab traffic; the other streams get
                            the rest of the chip).  2 = beside a MIRROR chain doing the same work (the two-chain CycleGAN step):
                            the K-split target is halved as well. */
  const GanAdamFuse* adam_fuse; /* optional, see above */
  void* dw_wire;         /* optional (data-parallel steps, no counterpart in the single-device reference): the bfloat16 wire buffer of the
                            gradient exchange at this kernel's offset ([16][big_c][small_c], 8-byte aligned).  When gan_wgrad_wire_direct()
                            returns 1 the launch writes the gradient there in the wire format (gan_grad_pack's rounding) and leaves dw
                            untouched: no fp32 gradient, no cast pass.  Not together with adam_fuse / accumulate; a launch whose plan
                            cannot honour a non-NULL dw_wire returns GAN_E_SHAPE. */
} GanWgradDesc;
/* Kernel gradient of Conv2D / Conv2DTranspose (GradientTape.gradient w.r.t. trainable_variables,
 * pix2pix.py:210-211, cycle_gan.py:252-260). */
int gan_conv_wgrad(const GanWgradDesc* d, gan_stream_t stream);
size_t gan_wgrad_workspace_bytes(const GanWgradDesc* d);
int gan_wgrad_plan_info(const GanWgradDesc* d, int32_t* info /* {TA, TB, splitM, fold} */);
int gan_wgrad_adam_fused(const GanWgradDesc* d);   /* 1: d->adam_fuse will be honoured, 0: not, < 0: error code */
int gan_wgrad_wire_direct(const GanWgradDesc* d);  /* 1: d->dw_wire will be honoured, 0: not, < 0: error code */

/* Produce typed NK copies from a fp32 Keras-layout master [16][A][B]:
 * nk_native [16][A][pad8(B)] and nk_transposed [16][B][pad8(A)] (either may be NULL). */
int gan_weights_prepare(const float* master, int32_t A, int32_t B, int32_t dtype,
                        void* nk_native, void* nk_transposed, gan_stream_t stream);

/* The same for every kernel of a network in one launch.  entries_dev: device array of n GanPrepEntry; tile_start =
 * running sum of 16 * ceil(pad8(A)/64) * ceil(pad8(B)/64) over the preceding entries, tiles_b = ceil(pad8(B)/64). */
typedef struct GanPrepEntry {
  const float* master; void* nk_native; void* nk_transposed;
  int32_t A, B, tile_start, tiles_b;
} GanPrepEntry;
int gan_weights_prepare_multi(const void* entries_dev, int32_t n, int32_t total_tiles, int32_t dtype, gan_stream_t stream);
/* Keras Adam (base_gan.py:247-252) fused with the above for the kernel tensors of a network: every listed tensor (its
 * master pointer must lie inside the flat `master` buffer; m / v / grad are indexed at the same offset) is updated in
 * TF form and its NK copies rewritten in the same pass.  gan_adam_begin must have run this step; non-kernel parameters
 * (norm scales/offsets, biases) are updated with gan_adam_tf.  All four buffers 16-byte aligned. */
int gan_adam_prepare_multi(const void* entries_dev, int32_t n, int32_t total_tiles, int32_t dtype, float* master, float* m,
                           float* v, const void* grad, const float* lr_t, float beta1, float beta2, float eps,
                           float grad_scale, const float* scale_state, int32_t grad_bf16, gan_stream_t stream);

/* Inference mode (training=False): Keras BatchNormalization with its moving statistics (base_gan.py:83,113,151 called with
 * training=False), y = gamma * (x - moving_mean) * rsqrt(moving_variance + eps) + beta, folded into the bias-free convolution
 * in front of it (base_gan.py:77-79, :106-110, :145-148).  Per output channel co, in fp32 without contraction:
 *     s[co] = gamma[co] * rsqrt(moving_var[co] + eps),   bias[co] = beta[co] - moving_mean[co] * s[co]
 *     nk[tap][co][ci] = dtype(master(tap, co, ci) * s[co])        (pad8(Cin) columns written as zeros)
 * so that the layer becomes ONE convolution launch with bias + activation in its epilogue.  `nk` has the layout the forward
 * entry point reads, [16][Cout][pad8(Cin)]: transposed = 1 for a Conv2D (HWIO master [16][A = Cin][B = Cout], the
 * gan_weights_prepare transposed copy), 0 for a Conv2DTranspose ((kh,kw,cout,cin) master [16][A = Cout][B = Cin], the native
 * copy).  Writes only `bias` and `nk` (buffers of the caller's inference path: never the NK copies the training step reads);
 * master, gamma, beta, moving_mean and moving_var are read only.  master and nk 16-byte aligned.
 * tile_start = running sum of 16 * ceil(Cout/64) * tiles_k over the preceding entries, tiles_k = ceil(pad8(Cin)/64). */
typedef struct GanFoldEntry {
  const float* master;
  const float* gamma;
  const float* beta;
  const float* moving_mean;
  const float* moving_var;
  float* bias;               /* [Cout] written */
  void* nk;                  /* [16][Cout][pad8(Cin)] written, dtype */
  int32_t A, B;              /* master dimensions, as GanPrepEntry */
  int32_t transposed;
  int32_t tile_start, tiles_k;
} GanFoldEntry;
/* Every BatchNorm-carrying kernel of a network in one launch (device array of n GanFoldEntry).  Enqueue-only, hipGraph-capturable. */
int gan_bn_fold_multi(const void* entries_dev, int32_t n, int32_t total_tiles, int32_t dtype, float eps, gan_stream_t stream);

/* ---- normalisation + activation ------------------------------------------------------------- */
typedef struct GanNormDesc {
  uint32_t struct_size;  /* sizeof(GanNormDesc) of the caller's build */
  int32_t dtype;
  GanTensor y;              /* raw convolution output */
  GanTensor a;              /* out: act(dropout(gamma * (y - mean) * rstd + beta)) */
  int32_t groups;           /* statistics groups over the batch dimension: 1 = BatchNormalization over the
                               whole batch (base_gan.py:83,113,151); y.n = InstanceNormalization
                               (utils.py:26-30); 2 = two BatchNormalization calls (D(real), D(fake),
                               pix2pix.py:202-203) batched into one launch */
  float eps;                /* 1e-3 Keras BN default; 1e-5 utils.py:9 */
  const float* gamma;       /* [c] gamma / scale */
  const float* beta;        /* [c] beta / offset */
  float* mean;              /* [groups][c] */
  float* rstd;              /* [groups][c] */
  float* moving_mean;       /* optional [c]: BN moving averages, updated once per group in order */
  float* moving_var;
  float momentum;           /* 0.99 */
  const uint8_t* dropmask;  /* optional [n*h*w*c] 0/1; survivors x2 (Dropout(0.5), base_gan.py:117-118) */
  int32_t act;
  float slope;
  void* workspace;          /* >= gan_norm_workspace_bytes() */
  size_t workspace_bytes;
  uint32_t* sync;           /* optional: gan_norm_sync_bytes() of device memory, zero when first used and owned by this
                               layer invocation (launches that share an area must be stream-ordered; the area zeroes
                               itself again): lets gan_norm_finalize_act_fwd() run as ONE launch */
} GanNormDesc;
int gan_norm_stats(const GanNormDesc* d, gan_stream_t stream);
/* finalize only: d->workspace already holds `chunks` partials per group written by a convolution epilogue */
int gan_norm_stats_finalize(const GanNormDesc* d, int32_t chunks, gan_stream_t stream);
int gan_norm_act_fwd(const GanNormDesc* d, gan_stream_t stream);
size_t gan_norm_workspace_bytes(int32_t groups, int32_t c, int64_t rows_per_group);
/* The same Keras layer call (base_gan.py:83-87, 113-120, 151-155; utils.py:26-30) in two steps whose second one is a single
 * launch: gan_norm_stats_partial() = the partial sums of gan_norm_stats() without its finalize launch;
 * gan_norm_finalize_act_fwd() = gan_norm_stats_finalize(d, chunks) + gan_norm_act_fwd(d), bit-identical to that pair
 * (chunks <= 0: the partials gan_norm_stats_partial() wrote).  With d->sync the finalize rides inside the apply launch:
 * its first workgroups finalize and publish mean / rstd (+ the moving averages), the others wait for them with their rows'
 * loads already in flight (option norm.fin_in_apply, default 1; without a sync area, or when the apply grid has fewer
 * workgroups than the finalize has work units: two launches).  Every wait is bounded; gan_norm_sync_error_offset() locates the flag a
 * timed-out wait leaves in the area. */
int gan_norm_stats_partial(const GanNormDesc* d, gan_stream_t stream);
int gan_norm_finalize_act_fwd(const GanNormDesc* d, int32_t chunks, gan_stream_t stream);
size_t gan_norm_sync_bytes(void);
/* byte offset, inside a sync area, of the 32-bit word that is non-zero after a wait timed out (host reads it after a sync) */
size_t gan_norm_sync_error_offset(void);

typedef struct GanNormBwdDesc {
  uint32_t struct_size;  /* sizeof(GanNormBwdDesc) of the caller's build */
  int32_t dtype;
  GanTensor y;              /* raw convolution output saved by forward */
  GanTensor da;             /* upstream gradient w.r.t. a */
  GanTensor da2;            /* optional second upstream (ptr NULL if absent): skip-connection gradient */
  GanTensor dy;             /* out: gradient w.r.t. y */
  int32_t groups;
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* rstd;
  const uint8_t* dropmask;
  int32_t act;
  float slope;
  float* dgamma;            /* optional [c] */
  float* dbeta;
  int32_t accumulate;       /* dgamma/dbeta += */
  void* workspace;
  size_t workspace_bytes;
  uint32_t* sync;           /* optional sync area (GanNormDesc.sync): the apply launch of gan_norm_act_bwd() /
                               gan_norm_act_bwd_fused() then also finalizes the sums, dgamma and dbeta (one launch less) */
} GanNormBwdDesc;
int gan_norm_act_bwd(const GanNormBwdDesc* d, gan_stream_t stream);
/* The same layer backward when its first half already ran in the producing dgrad's epilogue (GanBwdFuse above): d->da holds
 * dz (da2, dropmask, act are ignored / must be NULL), d->workspace the producer's partial sums, `chunks` per group as
 * reported by gan_conv_plan_info()[4], followed by room for [groups][c][2] floats.  Finalize + apply: dy, dgamma, dbeta. */
int gan_norm_act_bwd_fused(const GanNormBwdDesc* d, int32_t chunks, gan_stream_t stream);

typedef struct GanActBwdDesc { /* layers without normalisation: conv -> [bias] -> act */
  uint32_t struct_size;  /* sizeof(GanActBwdDesc) of the caller's build */
  int32_t dtype;
  GanTensor a;              /* saved activation output (sign for LeakyReLU, value for tanh) */
  GanTensor da;
  GanTensor da2;            /* optional */
  GanTensor dy;             /* out */
  int32_t act;
  float slope;
  float* dbias;             /* optional [c] (sum of dy over n,h,w) */
  int32_t accumulate;
  void* workspace;
  size_t workspace_bytes;
} GanActBwdDesc;
int gan_act_bwd(const GanActBwdDesc* d, gan_stream_t stream);

/* ---- losses --------------------------------------------------------------------------------- */
/* tf.keras.losses.BinaryCrossentropy(from_logits=True) against a constant target (base_gan.py:227-245).
 * x: fp32 logits [count]. loss_out[0] (+)= loss_scale * mean(bce). If dx != NULL:
 * dx[i*dx_pitch] = grad_scale * (sigmoid(x)-target)/count in `dtype`.  workspace >= 1024 floats (block partial
 * sums, added in a fixed order by a finalize launch). */
int gan_bce_logits(const float* x, int64_t count, float target, float loss_scale, int32_t loss_accumulate,
                   float* loss_out, float grad_scale, int32_t dtype, void* dx, int32_t dx_pitch, float* workspace,
                   const float* scale_state, gan_stream_t stream);
/* The three BCE terms of one Pix2Pix / PatchGAN step in one pass (generator_loss pix2pix.py:167-188 and
 * discriminator_loss base_gan.py:227-245 with the 0.5 of pix2pix.py:206): gan_loss = BCE(1, fake),
 * disc_loss = 0.5*(BCE(1, real) + BCE(0, fake)), gradients (optional, `dtype`, element stride `pitch`):
 * g_dfake = d gan_loss / d fake, d_dreal / d_dfake = d disc_loss / d real, fake.  If gen_total != NULL it receives
 * gan_loss + lambda * (*l1) (l1 = the already computed L1 term, pix2pix.py:184).  workspace >= 768 floats. */
int gan_patchgan_losses(const float* real_logits, const float* fake_logits, int64_t count, int32_t dtype, void* g_dfake,
                        void* d_dreal, void* d_dfake, int32_t pitch, float lambda, const float* l1, float* gen_total,
                        float* gan_loss, float* disc_loss, float* workspace, const float* scale_state, gan_stream_t stream);
/* Least-squares GAN objective (gan_loss 'lsgan'): the arguments of gan_bce_logits, one for one.
 * x: fp32 logits [count] (unbounded). loss_out[0] (+)= loss_scale * mean((x-target)^2). If dx != NULL:
 * dx[i*dx_pitch] = grad_scale * ls * 2*(x[i]-target)/count in `dtype`, ls = scale_state[0] or 1.  workspace >= 1024
 * floats (block partial sums, added in a fixed order by a finalize launch). */
int gan_lsq_logits(const float* x, int64_t count, float target, float loss_scale, int32_t loss_accumulate,
                   float* loss_out, float grad_scale, int32_t dtype, void* dx, int32_t dx_pitch, float* workspace,
                   const float* scale_state, gan_stream_t stream);
/* The three least-squares terms of one Pix2Pix / PatchGAN step in one pass; the arguments of gan_patchgan_losses, one
 * for one: gan_loss = mean((fake-1)^2), disc_loss = 0.5*(mean((real-1)^2) + mean(fake^2)), gradients (optional,
 * `dtype`, element stride `pitch`, each times ls): g_dfake = 2(fake-1)/count, d_dreal = (real-1)/count,
 * d_dfake = fake/count.  If gen_total != NULL it receives gan_loss + lambda * (*l1), two roundings.
 * workspace >= 768 floats. */
int gan_patchgan_losses_lsq(const float* real_logits, const float* fake_logits, int64_t count, int32_t dtype, void* g_dfake,
                            void* d_dreal, void* d_dfake, int32_t pitch, float lambda, const float* l1, float* gen_total,
                            float* gan_loss, float* disc_loss, float* workspace, const float* scale_state, gan_stream_t stream);
/* tf.reduce_mean(tf.abs(a - b)) (pix2pix.py:181, cycle_gan.py:167,176). loss_out (+)= loss_scale*mean.
 * da (optional, dtype, own pitch) = grad_scale * sign(a-b)/count. workspace >= 4096 floats. */
int gan_l1(int32_t dtype, const GanTensor* a, const GanTensor* b, float loss_scale, int32_t loss_accumulate,
           float* loss_out, float grad_scale, const GanTensor* da, float* workspace, const float* scale_state,
           gan_stream_t stream);

/* out[k] = a[k] + b[k] + c[k], n <= 64 device scalars: total_gen_g_loss = gen_g_loss + total_cycle_loss + identity_loss
 * (cycle_gan.py:243-244) without leaving the captured step. */
int gan_sum3(const float* a, const float* b, const float* c, float* out, int32_t n, gan_stream_t stream);

/* ---- optimiser ------------------------------------------------------------------------------ */
/* tf.keras.optimizers.Adam (base_gan.py:247-252), TF form: lr_t = lr*sqrt(1-b2^t)/(1-b1^t);
 * m += (g-m)(1-b1); v += (g*g-v)(1-b2); p -= lr_t*m/(sqrt(v)+eps).  `step` is a device counter:
 * gan_adam_begin increments it and writes lr_t, so a captured graph advances correctly on replay.  `lr` is a by-value
 * argument: a captured graph holds it for good.  A rate that changes during the run: gan_adam_begin_sched below. */
int gan_adam_begin(int32_t* step, float* lr_t, float lr, float beta1, float beta2, const float* scale_state, gan_stream_t stream);
/* Linear learning-rate decay as a function of the device step counter (no counterpart in the reference, whose rate is constant; the
 * Pix2Pix / CycleGAN papers' schedule): update index i = t - 1 (0-based) runs at lr * f(i),
 *   f(i) = 1                                                                       i <  decay_start
 *        = end_factor + (1 - end_factor) * (decay_end - i) / (decay_end - decay_start)   decay_start <= i < decay_end
 *        = end_factor                                                              i >= decay_end
 * so f(decay_start) = 1 (no jump) and the last decayed update, decay_end - 1, is still above the floor. */
typedef struct GanLrSchedule {
  uint32_t struct_size;
  float    lr;           /* base learning rate */
  float    end_factor;   /* share of lr that is left from decay_end on, 0 ..= 1 */
  int32_t  decay_start;  /* first 0-based update index that is decayed */
  int32_t  decay_end;    /* from this update index on: lr * end_factor */
} GanLrSchedule;
/* gan_adam_begin with the rate of the schedule: t = *step + 1 is stored, lr_now (device, one float, may be NULL) receives
 * (float)(lr * f(t - 1)) and lr_t (float)(lr * f(t - 1) * sqrt(1-b2^t)/(1-b1^t)), double arithmetic from the fp32 arguments, one
 * rounding each; where f = 1 lr_t has the bits gan_adam_begin writes, where f = 0 both are +0.  A skipped step (scale_state[3] != 0)
 * leaves step, lr_t and lr_now alone.  The schedule is read at enqueue (a captured graph holds it by value) and advances with the
 * counter on replay.  GAN_E_ARG and no launch: NULL step / lr_t / s, a struct_size this library was not built with, lr not finite
 * or <= 0, end_factor outside [0, 1], decay_start < 0, decay_end <= decay_start. */
int gan_adam_begin_sched(int32_t* step, float* lr_t, float* lr_now, const GanLrSchedule* s, float beta1, float beta2,
                         const float* scale_state, gan_stream_t stream);
/* grad: fp32 [count], or with grad_bf16 != 0 the bfloat16 wire buffer of the data-parallel exchange (gan_grad_pack, summed
 * over ranks): Adam then reads the exchanged gradient where it landed, grad_scale = 1/world (8-byte aligned). */
int gan_adam_tf(float* param, float* m, float* v, const void* grad, int64_t count, const float* lr_t,
                float beta1, float beta2, float eps, float grad_scale, const float* scale_state, int32_t grad_bf16,
                gan_stream_t stream);

/* Dynamic loss scaling for the fp16 path (GAN_F16; the reference trains in fp32 and has none - this is what
 * tf.keras.mixed_precision.LossScaleOptimizer would add around base_gan.py:247-252).  scale_state: 4 floats on the
 * device {scale, 1/scale, finite steps in a row, this step's gradients are non-finite}.  Every loss entry point above
 * multiplies the GRADIENTS it writes by scale (reported losses stay unscaled); every Adam entry point multiplies the
 * gradients it reads by 1/scale and does nothing - gan_adam_begin included - while the non-finite flag is set.
 * Per step: backward -> gan_grads_check on each gradient buffer -> Adam -> gan_loss_scale_update (halves the scale after
 * a non-finite step, doubles it after growth_interval finite ones, clears the flag).  scale_state == NULL everywhere:
 * no scaling (fp32 / bf16 paths). */
int gan_grads_check(const float* grad, int64_t count, float* scale_state, gan_stream_t stream);
int gan_loss_scale_update(float* scale_state, int32_t growth_interval, float max_scale, gan_stream_t stream);

/* Exponential moving average of a weight arena (no counterpart in the reference; tf.train.ExponentialMovingAverage's update):
 * shadow <- shadow + (param - shadow) * (1 - d_t), per element as fmaf(param - shadow, 1 - d_t, shadow).
 * d_t = decay if step == NULL, else min(decay, (1 + t) / (10 + t)) with t = *step (the num_updates form: a young average
 * follows the weights closely); `step` is the device counter gan_adam_begin advances and is only read here.  decay_used
 * (device, one float, may be NULL) receives d_t.  One streaming launch, no atomics, no workspace: the same inputs give the
 * same bits.  count > 0 and a multiple of 4, both arrays 16-byte aligned, 0 <= decay < 1; otherwise GAN_E_ARG and no launch. */
int gan_ema_update(float* shadow, const float* param, int64_t count, float decay, const int32_t* step, float* decay_used,
                   gan_stream_t stream);

/* ---- misc ----------------------------------------------------------------------------------- */
/* Bernoulli(0.5) keep-mask from a counter hash of (seed, *step, stream_id, index). */
int gan_dropout_mask(uint8_t* mask, int64_t count, uint64_t seed, const int32_t* step, uint32_t stream_id,
                     gan_stream_t stream);
/* the same for n <= 4 masks (the three Dropout layers of a generator call) in a single launch; host arrays.  draws: optional
 * device int32[2], zero-initialised by the caller: a per-call-site launch counter mixed into the hash and advanced by the
 * launch itself, so that successive calls draw new masks while *step stands still (training=True forward passes of the
 * validation loop, pix2pix.py:228 / :338: Keras draws a fresh mask per call).  NULL = the single-mask hash above. */
int gan_dropout_mask_multi(int32_t n, uint8_t* const* masks, const int64_t* counts, uint64_t seed, const int32_t* step,
                           const uint32_t* stream_ids, int32_t* draws, gan_stream_t stream);
/* dst(dtype, pitch view) <- src fp32 dense [n,h,w,c]  /  dst fp32 dense <- src(dtype, pitch view) */
int gan_pack(int32_t dtype, const float* src, const GanTensor* dst, gan_stream_t stream);
/* n <= 4 (source, destination) pairs of one shape in a single launch (host arrays, read at call time) */
int gan_pack_multi(int32_t dtype, int32_t n, const float* const* srcs, const GanTensor* dsts, gan_stream_t stream);
int gan_unpack(int32_t dtype, const GanTensor* src, float* dst, gan_stream_t stream);
/* typed view -> typed view (same n,h,w,c; pitches / channel offsets may differ): places the generator
 * output into the discriminator's concat input (base_gan.py:139) and routes its gradient back. */
int gan_copy_view(int32_t dtype, const GanTensor* src, const GanTensor* dst, gan_stream_t stream);
/* Image history pool of a discriminator (no counterpart in the reference; Zhu et al. 2017, section 4 after Shrivastava et al.:
 * the discriminator is trained on a history of generated images).  One query takes the n = src.n current images in batch order:
 *     for b in 0 .. n-1:   if stored < capacity:  pool[stored] = img[b]; out[b] = img[b]; stored += 1        (fill)
 *                          elif swap(b):          j = slot(b); out[b] = pool[j]; pool[j] = img[b]              (swap)
 *                          else:                  out[b] = img[b]                                              (keep)
 *     key = mix64(seed ^ ((uint64)(uint32)launches << 32) ^ stream_id),  h = mix64(key ^ b)       (the dropout masks' counter hash)
 *     swap(b) = h >> 63,   slot(b) = ((h & 0xffffffff) * capacity) >> 32
 * `launches` is the pool's own counter, not an Adam step counter: a skipped fp16 step still advances the pool.  The sequential
 * semantics hold exactly, also for several images of one batch that pick the same slot (a thread owns its element positions in
 * every image and every slot).  Bits are moved, nothing is computed.  One launch; enqueue-only and capturable: the state lives on
 * the device and advances on replay. */
typedef struct GanPoolDesc {
  uint32_t struct_size;
  int32_t dtype;               /* GAN_F32 | GAN_BF16 | GAN_F16: storage of src, dst and pool */
  GanTensor src;               /* the n current images (the generator's output view): only read */
  GanTensor dst;               /* out: same n, h, w, c, own pitch (a slot of the discriminator's input); only the c real channels of
                                  a pixel are written, the pad channels of a wider pitch keep what they hold */
  void* pool;                  /* device: dense [capacity][h][w][c] of dtype; only the filled or swapped slots are written */
  int32_t capacity;            /* >= 1 */
  uint32_t stream_id;          /* tells the pools of one seed apart */
  uint64_t seed;
  int32_t* state;              /* device int32[3], zero-initialised by the caller: {stored, launches, block ticket}; every workgroup
                                  reads it before it takes a ticket, the last ticket holder stores min(capacity, stored + n) and
                                  launches + 1 and clears the ticket */
} GanPoolDesc;
/* 16-byte accesses where src, dst and pool are dense runs (pitch == c, h * w * c * element size a multiple of 16, 16-byte aligned
 * pointers); element accesses placed by (pixel, channel) otherwise - the 8-channel-padded views with c = 1 or 3.
 * GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, capacity < 1, n / h / w / c of src and dst differ or are < 1, pitch < c,
 * a pointer not aligned to its element size.  GAN_E_SHAPE: h * w * pitch of an image >= 2^31.  All found before the launch. */
int gan_pool_exchange(const GanPoolDesc* d, gan_stream_t stream);
/* Differentiable augmentation of what a discriminator sees (no counterpart in the reference; Zhao et al., "Differentiable
 * Augmentation for Data-Efficient GAN Training", NeurIPS 2020): colour (brightness, saturation), then
 * translation with zero fill, then cutout, per image, the same family on real and generated inputs, and the exact transpose of
 * that map for the generator's gradient.  One record per image of a discriminator invocation, in device memory: */
typedef struct GanDiffAugParams {   /* 32 bytes */
  int32_t tx, ty;                   /* translation in pixels (tx along w, ty along h): y(p) reads x(p - t) */
  int32_t cut_x0, cut_y0, cut_w, cut_h;  /* cut rectangle in OUTPUT coordinates, already clipped to the image; cut_w = 0: none */
  float brightness;                 /* added to every real channel */
  float saturation;                 /* s: x_c -> (x_c - m) * s + m, m = mean over the channels of the pixel's own image */
} GanDiffAugParams;
enum { GAN_DIFFAUG_TRANSLATION = 1, GAN_DIFFAUG_CUTOUT = 2, GAN_DIFFAUG_BRIGHTNESS = 4, GAN_DIFFAUG_SATURATION = 8 };
/* Host only: "translation,cutout" (any comma-separated subset of translation, cutout, brightness, saturation; "" = none) -> the
 * policy bit mask.  GAN_E_ARG: NULL names / policy, an unknown or empty name. */
int gan_diffaug_policy(const char* names, uint32_t* policy);
/* params[0 .. n-1] <- fresh draws for images of h x w pixels, then *launches += 1.  One launch of one workgroup; enqueue-only and
 * capturable: `launches` (device int32, zero-initialised by the caller) is the draws' own counter - not an Adam step counter -
 * every thread reads it before the one store that advances it, so a replayed graph draws anew.  Bit layout of the draws
 * (mix64 = the dropout masks' counter hash; lo(h) = h & 0xffffffff, hi(h) = h >> 32, both as uint64):
 *     key = mix64(seed ^ ((uint64)(uint32)launches << 32) ^ stream_id),   h_k = mix64(key ^ (uint64)(4 * i + k)) for record i
 *     translation: Tx = (w + 4) / 8, Ty = (h + 4) / 8 (integer division: round(size / 8));
 *                  tx = (int)((lo(h_0) * (2 Tx + 1)) >> 32) - Tx,   ty = (int)((hi(h_0) * (2 Ty + 1)) >> 32) - Ty
 *     cutout:      per axis (x: size = w, 32 bits = lo(h_1); y: size = h, 32 bits = hi(h_1)):  cs = size / 2,
 *                  N = size + (1 - cs % 2),  off = (bits * N) >> 32  (uniform on 0 .. N-1, the centre offset of the paper's code),
 *                  start = off - cs / 2;  the rectangle [start, start + cs) intersected with [0, size): cut_x0 / cut_w, cut_y0 / cut_h
 *                  (never empty for size >= 2; size = 1: cs = 0, nothing is cut, cut_w = cut_h = 0)
 *     brightness:  (float)(h_2 >> 40) * 2^-24 - 0.5     in [-0.5, 0.5), exact in fp32
 *     saturation:  (float)(h_3 >> 40) * 2^-23           in [0, 2), exact in fp32
 * A policy whose bit is not set in `policy` writes its neutral value: tx = ty = 0; cut_x0 = cut_y0 = cut_w = cut_h = 0;
 * brightness = 0; saturation = 1.
 * GAN_E_ARG and no launch: NULL params / launches, n < 1 or n > 128, h or w < 1, policy bits beyond the four, params not 4-byte
 * aligned, launches not 4-byte aligned. */
int gan_diffaug_draw(GanDiffAugParams* params, int32_t n, int32_t h, int32_t w, uint32_t policy, uint64_t seed,
                     uint32_t stream_id, int32_t* launches, gan_stream_t stream);
/* One direction of the map for the images of a view.  With P = params[sample0 + b] for image b, p a pixel, ch a channel:
 *   forward  (direction 0):  y(p, ch) = cut(p) ? 0 : (p - t inside the image ? colour(x(p - t, ch)) : 0)
 *                            colour(x_ch) = (x_ch - m) * s + m + brightness,   m = mean of the group's channels at that pixel
 *                            (group_c = 1: m = x_ch and s drops out: x_ch + brightness)
 *   backward (direction 1):  dx(q, ch) = (q + t inside the image and not cut(q + t)) ? s * dy(q + t, ch) + (1 - s) * mean_group(dy(q + t, .)) : 0
 *                            (src = dy, dst = dx; group_c = 1: dy(q + t, ch))
 * cut(p) = cut_w > 0 and cut_x0 <= p.x < cut_x0 + cut_w and cut_y0 <= p.y < cut_y0 + cut_h.  The backward direction is the exact
 * transpose of the forward one and a gather as well: no atomics, the same inputs give the same bits.  Arithmetic in fp32
 * (m = (x_0 + x_1 + x_2) / 3, one fused multiply-add, one add), rounded once to the storage dtype; where colour is the identity
 * (forward: brightness = 0 and, for group_c = 3, s = 1; backward: s = 1 or group_c = 1) bits are moved and nothing is computed;
 * the fill is +0.  Only the c real channels of dst are written: pad channels of a wider pitch and memory outside the view keep
 * their bits; pad channels of src are never used (they may hold NaN).  src and dst must not overlap.  One launch, enqueue-only and
 * capturable, no workspace. */
typedef struct GanDiffAugDesc {
  uint32_t struct_size;
  int32_t dtype;               /* GAN_F32 | GAN_BF16 | GAN_F16: storage of src and dst */
  GanTensor src;               /* n images of h x w, c channels, own pitch: only read */
  GanTensor dst;               /* out: same n, h, w, c, own pitch */
  int32_t group_c;             /* 1 or 3: channels of one image; c is a multiple of it ([input | target] with c = 2 * group_c is two
                                  images per sample: saturation is taken inside each group) */
  int32_t sample0;             /* image b of the view uses params[sample0 + b]; >= 0 */
  const GanDiffAugParams* params;   /* device: at least sample0 + n records; only read */
  int32_t direction;           /* 0 forward, 1 backward (transpose) */
} GanDiffAugDesc;
/* A thread owns a pixel.  Where a pixel of src is one aligned 16-byte unit (pitch * element size = 16, 16-byte aligned src.ptr,
 * c within it: the step's bf16 / fp16 buffers of pitch 8, fp32 of pitch 4) it is fetched with one 16-byte load; element loads
 * placed by (pixel, channel) otherwise.  dst is always written by elements, channel by channel: launches that fill other channels
 * of the same pixels (the generated channels beside the input channels of a discriminator input) may run beside this one.
 * GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, n / h / w / c of src and dst differ or are < 1, pitch < c, group_c not 1
 * or 3, c not a multiple of group_c, sample0 < 0, direction not 0 or 1, a tensor pointer not aligned to its element size, params
 * not 4-byte aligned.  GAN_E_SHAPE: h * w * pitch of an image >= 2^31, n > 65535.  All found before the launch. */
int gan_diffaug_apply(const GanDiffAugDesc* d, gan_stream_t stream);
/* bias gradient: dbias[c] (+)= sum over n,h,w of dy[...,c]; dy.c 8-padded, dbias has dy.c entries.
 * workspace >= gan_norm_workspace_bytes(1, dy.c, n*h*w). */
int gan_bias_grad(int32_t dtype, const GanTensor* dy, float* dbias, int32_t accumulate, void* workspace,
                  size_t workspace_bytes, gan_stream_t stream);
/* Wire format of the data-parallel gradient exchange (no counterpart in the reference, which is single-device:
 * base_gan.py:18-19 only prints the GPU count; semantics in SURVEY.md section 8e): fp32 gradients -> bf16 wire buffer
 * before the RCCL all-reduce, and back (times `scale` = 1/world) before Adam.  count % 8 == 0, 16-byte aligned. */
int gan_grad_pack(const float* src, void* dst_bf16, int64_t count, gan_stream_t stream);
int gan_grad_unpack(const void* src_bf16, float* dst, int64_t count, float scale, gan_stream_t stream);

/* ---- device-resident input pipeline ------------------------------------------------------------ */
/* The reference's tf.data map after the decode (pix2pix.py:34-87 / cycle_gan.py:40-72, base_gan.py:46-61: left/right split,
 * nearest-neighbour resize to size+30, random crop, random mirror, v / 127.5 - 1), for uint8 images that stay in device memory:
 * an integer gather through host-built index tables plus one 256-entry value table.
 *     dst[i][r][x][ch] = lut[ src[src_offset + rows[crop_y + r] * src_pitch + (col0 + cols[crop_x + x']) * c + ch] ],
 *     x' = flip ? out - 1 - x : x,   rows = tables + row_table * table_len,   cols = tables + col_table * table_len
 * One GanAugSample per output image, in a HOST array that is read at call time (nothing of it has to outlive the call; no
 * per-step upload).  dst_b (optional) is a second tensor of the same shape built from the same rows, crop and mirror but from
 * the columns col0_b + (table col_table_b): both images of a Pix2Pix pair in one launch.  The table entries are trusted to lie inside
 * the image (the caller built them from its size); every read is additionally clamped to [0, src_bytes). */
typedef struct GanAugSample {
  int64_t src_offset;  /* byte offset of the image's first pixel in src */
  int32_t src_pitch;   /* bytes between consecutive source rows */
  int32_t col0;        /* first source column (pixels) of the part that goes to dst_a; the split: 0 or width / 2 */
  int32_t col0_b;      /* the same for dst_b (unused without dst_b) */
  int32_t row_table;   /* table number of the row map, 0 <= . < n_tables */
  int32_t col_table;   /* table number of the column map of dst_a */
  int32_t col_table_b; /* the same for dst_b: the halves of an odd-width pair differ by one column (unused without dst_b) */
  int32_t crop_y;      /* crop origin in the table: 0 <= crop_y <= table_len - out */
  int32_t crop_x;
  int32_t flip;        /* 1: mirrored left-right */
} GanAugSample;

enum { GAN_AUGMENT_MAX_SAMPLES = 64 };

typedef struct GanAugmentDesc {
  uint32_t struct_size;
  int32_t n;                   /* samples of this launch, 1 ..= GAN_AUGMENT_MAX_SAMPLES */
  int32_t out;                 /* output height = width: 256 or 512 */
  int32_t c;                   /* channels, interleaved in the source: 1 or 3 */
  const uint8_t* src;          /* device: the packed uint8 images; 16-byte aligned */
  int64_t src_bytes;           /* size of that buffer, a multiple of 16 */
  const int32_t* tables;       /* device: n_tables index tables of table_len entries each */
  int32_t n_tables;
  int32_t table_len;           /* out + 30 for the jittered form, out for the plain resize (validation, test) */
  const float* lut;            /* device: 256 fp32 values, the normalised value of every byte */
  float* dst_a;                /* device: dense fp32 [n, out, out, c], 16-byte aligned */
  float* dst_b;                /* the pair's second tensor, or NULL */
  const GanAugSample* samples; /* HOST array of n entries */
} GanAugmentDesc;

/* GAN_E_ARG: NULL pointer, wrong struct_size, n out of range, c not 1 or 3, misaligned buffer, table number out of range,
 * source offset / pitch outside src.  GAN_E_SHAPE: out not 256 or 512, table_len < out, crop origin outside the table.  All of
 * them are found before anything is launched. */
int gan_augment_u8(const GanAugmentDesc* d, gan_stream_t stream);

/* Image preprocessing of the resident uint8 images, once, before any batch is built: the chain of the reference's curation script
 * (create_training_imgs/curate_FLIR_data.py: cv2.createCLAHE(clipLimit=1.0, tileGridSize=(15, 15)), a Gaussian blur of sigma
 * 0.5, a 3 x 3 sharpening filter), in place.  A REGION is a height x width window of a c-channel interleaved image with its own
 * row pitch (each half of a Pix2Pix pair is one); every channel is its own plane (per-channel equalisation, no colour-space
 * conversion).  A stage reads no byte outside its region: borders are reflect-101 of the region itself.  The stages run in the
 * fixed order CLAHE, blur, sharpen, each on the previous stage's bytes; the arithmetic is DESIGN.md section 25:
 *   CLAHE   OpenCV's 8-bit algorithm with tilesX = tilesY = grid: reflect-pad right / bottom to a multiple of grid, per tile a
 *           256-bin histogram, clipped at max(int(clip * area / 256), 1) (clip = 0: no clipping) and redistributed, a table
 *           rint(cumsum * float(255 / area)), then per pixel the bilinear blend of four tables in fp32 without contraction.
 *   blur    integer taps q[-r .. r] summing to 256 (r = (int(rint(6 sigma + 1)) | 1) / 2; q_i = rint(256 w_i), the centre takes the
 *           remainder), a horizontal and a vertical pass, out = (sum + 32768) >> 16.
 *   sharpen clamp(5 p - up - down - left - right, 0, 255).
 * clip and sigma are taken as the doubles their float values convert to.  Bytes of src outside the regions are not written.
 * Regions of one call must not overlap.  n may be any positive number: the regions travel to the kernels by value,
 * GAN_PREPROCESS_MAX_REGIONS per launch, and the launches of one group of regions reuse the workspace behind those of the group
 * before (stream order). */
typedef struct GanPreRegion {
  int64_t src_offset;  /* byte offset of the region's first byte (row 0, column 0, channel 0) in src */
  int32_t pitch;       /* bytes between consecutive rows, >= width * c */
  int32_t height;      /* rows */
  int32_t width;       /* pixels per row */
} GanPreRegion;

enum { GAN_PREPROCESS_MAX_REGIONS = 64 };
enum { GAN_PRE_CLAHE = 1, GAN_PRE_BLUR = 2, GAN_PRE_SHARPEN = 4 };

typedef struct GanPreprocessDesc {
  uint32_t struct_size;
  int32_t n;                   /* regions, >= 1 */
  int32_t c;                   /* channels, interleaved: 1 or 3 */
  uint32_t stages;             /* GAN_PRE_* bits, at least one */
  uint8_t* src;                /* device: the packed uint8 images */
  int64_t src_bytes;           /* size of that buffer */
  float clip;                  /* CLAHE clip limit, finite and >= 0 (0: no clipping) */
  int32_t grid;                /* CLAHE tiles per side, 1 ..= 32 */
  float sigma;                 /* blur: 0 < sigma <= 1.5 */
  void* workspace;             /* device: >= gan_preprocess_workspace_bytes(d), 16-byte aligned */
  size_t workspace_bytes;
  const GanPreRegion* regions; /* HOST array of n entries, read at call time */
} GanPreprocessDesc;

/* Bytes of workspace the call needs (the tile tables and one dense copy of each region, of the largest group of
 * GAN_PREPROCESS_MAX_REGIONS regions); 0 for a descriptor gan_preprocess_u8 refuses (src, workspace and src_bytes are not looked at). */
size_t gan_preprocess_workspace_bytes(const GanPreprocessDesc* d);
/* GAN_E_ARG: NULL pointer, wrong struct_size, n < 1, c not 1 or 3, stages 0 or with unknown bits, a region outside src or with
 * pitch < width * c, grid outside 1 .. 32, sigma outside (0, 1.5], clip negative or not finite, workspace not 16-byte aligned.
 * GAN_E_SHAPE: a side shorter than grid (CLAHE), than r + 1 (blur) or than 2 (sharpen), or (height - 1) * pitch + width * c >= 2^31.
 * GAN_E_WORKSPACE: workspace too small.  All found before anything is launched; enqueue-only. */
int gan_preprocess_u8(const GanPreprocessDesc* d, gan_stream_t stream);

/* ---- image-quality metrics ---------------------------------------------------------------------- */
/* Per image of a batch of pairs, on the display range u = 0.5 * x + 0.5 (the mapping generate_images plots, pix2pix.py:236; inputs in
 * [-1, 1], max_val = 1): out[i] = {ssim, psnr, mae, mse}.
 *   ssim = tf.image.ssim(u_a, u_b, max_val=1, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03): Gaussian window applied
 *          separably with VALID padding (map (h-10) x (w-10)); per channel lum * cs with
 *          lum = (2 mx my + c1) / (mx^2 + my^2 + c1), cs = (2 F(ab) - 2 mx my + c2) / (F(a^2 + b^2) - mx^2 - my^2 + c2),
 *          c1 = 1e-4, c2 = 9e-4; mean over the map, then over the channels.  Exactly 1 for a == b.
 *   mae = mean |u_a - u_b|, mse = mean (u_a - u_b)^2 over h * w * c, psnr = -10 log10(mse) (tf.image.psnr; +inf for mse = 0).
 * The reference itself only ever calls tf.image.ssim on (input, target) (pix2pix.py:182-184); this is the measurement between the
 * generator's output and the target.  a and b: same n, h, w, c with c = 1 or 3, 11 <= h, w <= 4096, each of its own dtype and
 * pitch (a channel-slice view of a wider buffer is fine: only the c real channels are read).  Two launches: fp32 partial sums per
 * (image, 32 x 32 tile of the map) into the workspace, then one fixed-order sum per image - no atomics, bit-identical from call
 * to call, an image's row independent of the rest of the batch. */
typedef struct GanQualityDesc {
  uint32_t struct_size;
  int32_t dtype_a;             /* GAN_F32 | GAN_BF16 | GAN_F16: storage of a */
  int32_t dtype_b;             /* the same for b */
  GanTensor a;
  GanTensor b;
  float* out;                  /* device: [n][4] = {ssim, psnr, mae, mse} */
  void* workspace;             /* device: >= gan_image_quality_workspace_bytes(n, h, w, c), 4-byte aligned */
  size_t workspace_bytes;
} GanQualityDesc;
/* 0 for a shape gan_image_quality refuses */
size_t gan_image_quality_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, n / h / w / c of a and b differ, n < 1, pitch < c.
 * GAN_E_SHAPE: h or w below 11 or above 4096.  GAN_E_WORKSPACE: workspace too small.  All found before anything is launched. */
int gan_image_quality(const GanQualityDesc* d, gan_stream_t stream);

/* ---- structural dissimilarity as a training loss ------------------------------------------------- */
/* loss = 1 - mean_i ssim_i with ssim_i exactly the `ssim` column of gan_image_quality (same window, constants, display range and
 * centred arithmetic: loss is exactly 0 for a == b), and its gradient with respect to a (the prediction).  With mx = F(ua),
 * my = F(ub), sxy = F(ua ub), sq = F(ua^2 + ub^2), A1 = 2 mx my + c1, B1 = mx^2 + my^2 + c1, A2 = 2 (sxy - mx my) + c2,
 * B2 = sq - mx^2 - my^2 + c2, S = A1 A2 / (B1 B2) per map position and
 *   P = dS/dmx = (2 my A2 - 2 my A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2),  Q = dS/dsxy = 2 A1 / (B1 B2),  R = dS/dsq = -S / B2,
 *   dloss/da(p) = -0.5 / (n c |M|) * (G^T[P](p) + ub(p) G^T[Q](p) + 2 ua(p) G^T[R](p)),
 * G^T[Z](p) = sum over the valid map positions q, 0 <= p - q <= 10 per axis, of g(py - qy) g(px - qx) Z(q)   (DESIGN.md section 14).
 * No counterpart in the reference: its SSIM term compares the input with the target (pix2pix.py:182-184) and has no gradient.
 * Two launches: one workgroup per (image, 32 x 32 tile of pixels) writes da once per pixel and one fp32 partial sum of S into the
 * workspace, then one fixed-order sum (double) - no atomics, bit-identical from call to call, enqueue-only and capturable.  The
 * value written for an image is its batch-1 gradient divided by n, rounded once: it does not depend on the rest of the batch. */
typedef struct GanDssimDesc {
  uint32_t struct_size;
  int32_t dtype_a;             /* GAN_F32 | GAN_BF16 | GAN_F16: storage of a */
  int32_t dtype_b;             /* the same for b */
  GanTensor a;                 /* prediction: c = 1 or 3, own pitch; only the c real channels are read (pads may hold NaN) */
  GanTensor b;                 /* target: same n, h, w, c; own dtype and pitch */
  float loss_scale;
  int32_t loss_accumulate;     /* 0 | 1 */
  float* loss_out;             /* device: loss_out[0] (+)= loss_scale * loss, as gan_l1 */
  float grad_scale;
  int32_t dtype_da;            /* storage of da */
  GanTensor da;                /* ptr NULL: loss only.  da = grad_scale * [scale_state[0]] * dloss/da rounded to dtype_da; same n, h,
                                  w, c as a, own pitch; only the c real channels are written */
  void* workspace;             /* device: >= gan_dssim_workspace_bytes(n, h, w, c), 4-byte aligned */
  size_t workspace_bytes;
  const float* scale_state;    /* fp16 loss scaling, as every loss entry point; NULL = none */
} GanDssimDesc;
/* 0 for a shape gan_dssim refuses */
size_t gan_dssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, n / h / w / c of a, b (and da) differ, n < 1, pitch < c,
 * loss_accumulate not 0 or 1.  GAN_E_SHAPE: h or w below 11 or above 4096.  GAN_E_WORKSPACE: workspace too small.  All found
 * before anything is launched. */
int gan_dssim(const GanDssimDesc* d, gan_stream_t stream);

/* ---- Sobel edge term of the generator loss --------------------------------------------------------- */
/* Mean absolute Sobel response of the difference image, and its gradient with respect to a (the prediction); DESIGN.md section 22.
 * No counterpart in the reference.  d = a - b in fp32 from the stored values; Sx = [[-1,0,1],[-2,0,2],[-1,0,1]], Sy = Sx^T, applied
 * as correlation at the valid positions q only (1 <= qy <= h-2, 1 <= qx <= w-2: nothing is padded or reflected), M = (h-2)(w-2):
 *   ex(q) = (Sx * d)(q) / 8,   ey(q) = (Sy * d)(q) / 8,
 *   loss = sum over images, channels and valid q of (|ex(q)| + |ey(q)|) / (2 n c M),
 *   dloss/da(p) = k(p) / (16 n c M),
 *   k(p) = sum over the valid q with |q - p|_inf <= 1 of Sx(p - q) sgn(ex(q)) + Sy(p - q) sgn(ey(q)),   sgn(0) = 0,
 * an integer in [-16, 16]; a pixel on the image's edge receives only the positions that exist.
 * Rounding order of the gradient: g = (float(k) * F) / float(n) with the ONE precomputed factor F = (float)(grad_scale / (16 c M))
 * (the batch-1 coefficient: the quotient in double from the fp32 grad_scale, rounded once), then g = g * scale_state[0] when
 * scale_state is given; the product, the quotient and the second product are each rounded to fp32 on their own.  So an image's
 * gradient at batch n is its batch-1 gradient divided by n, rounded once, as gan_dssim's.  grad_accumulate = 0: da = dtype_da(g).  grad_accumulate = 1: da = dtype_da(float(da_old) + g), one
 * fp32 addition, one rounding to the storage type.  Loss: per (image, tile) one fp32 partial sum of |ex| + |ey|, the partials added
 * in a fixed order in double, loss_out[0] (+)= (float)(sum / (2 n c M)) * loss_scale.
 * Two launches: one workgroup per (image, 32 x 32 tile of pixels) stages d with a 2-pixel halo in LDS, forms the two sign maps on
 * the tile plus 1, writes (or updates) every da element exactly once from its owner thread and writes one fp32 partial to the
 * workspace; then one fixed-order sum.  No atomics, bit-identical from call to call, enqueue-only, capturable, allocates nothing.
 * An image's gradient does not depend on the rest of the batch other than through the division by n. */
typedef struct GanEdgeDesc {
  uint32_t struct_size;
  int32_t dtype_a;             /* GAN_F32 | GAN_BF16 | GAN_F16: storage of a */
  int32_t dtype_b;             /* the same for b */
  GanTensor a;                 /* prediction: c = 1 or 3, own pitch; only the c real channels are read (pads may hold NaN) */
  GanTensor b;                 /* target: same n, h, w, c; own dtype and pitch */
  float loss_scale;
  int32_t loss_accumulate;     /* 0 | 1 */
  float* loss_out;             /* device: loss_out[0] (+)= loss_scale * loss, as gan_l1 */
  float grad_scale;
  int32_t dtype_da;            /* storage of da */
  GanTensor da;                /* ptr NULL: loss only.  Same n, h, w, c as a, own pitch; only the c real channels are read and written */
  void* workspace;             /* device: >= gan_edge_workspace_bytes(n, h, w, c), 4-byte aligned */
  size_t workspace_bytes;
  const float* scale_state;    /* fp16 loss scaling, as every loss entry point (the gradient only); NULL = none */
  int32_t grad_accumulate;     /* 0: da = g;  1: da = round(float(da) + g) - a second term on a gradient another loss wrote */
} GanEdgeDesc;
/* 0 for a shape gan_edge_l1 refuses */
size_t gan_edge_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, n / h / w / c of a, b (and da) differ, n < 1, pitch < c,
 * loss_accumulate or grad_accumulate not 0 or 1.  GAN_E_SHAPE: h or w below 3 or above 4096.  GAN_E_WORKSPACE: workspace too small.
 * All found before anything is launched. */
int gan_edge_l1(const GanEdgeDesc* d, gan_stream_t stream);

/* ---- multi-scale structural dissimilarity as a training loss (and a metric) ----------------------------- */
/* MS-SSIM (Wang, Simoncelli, Bovik 2003; tf.image.ssim_multiscale) of a (prediction) against b (target), its loss 1 - mean and
 * the gradient with respect to a; DESIGN.md section 24.  No counterpart in the reference.
 * Levels.  M = scales, 1 .. 5.  Level 0 is the stored image; level j + 1 has h' = ceil(h_j / 2), w' = ceil(w_j / 2) and is the
 * 2 x 2 mean with the last row / column repeated where a side is odd (symmetric padding, then a VALID average pool):
 *   x_{j+1}(i, k) = 0.25 * ((x_j(2i, 2k) + x_j(2i, k1)) + (x_j(i1, 2k) + x_j(i1, k1))),  i1 = min(2i + 1, h_j - 1),  k1 = min(2k + 1, w_j - 1),
 * in fp32 in that order on the centred values x' = 0.5 x that gan_dssim stages, by the same operations for a and b.
 * Shapes.  c = 1 or 3, h, w <= 4096 and h, w >= 11 * 2^(M - 1): every level holds a full window (h_j, w_j >= 11), also where it is
 * pooled without the repeated edge; anything else is GAN_E_SHAPE.
 * Per level, image and channel, with gan_dssim's lum = A1 / B1 and cs = A2 / B2 (same window, c1, c2, display range, VALID map):
 *   CS_j = mean over the map of cs,   S_j = mean over the map of lum * cs,
 *   MS = prod_{j < M-1} max(CS_j, 0)^power[j] * max(S_{M-1}, 0)^power[M-1],
 * an image's score is the channel mean of MS (per_image[i] when given) and loss = 1 - mean over the images.  With M = 1 and
 * power[0] = 1 this is gan_dssim's loss.
 * Gradient.  k_j = power[j] MS / CS_j (j < M-1), k_{M-1} = power[M-1] MS / S_{M-1}, every k of an image and channel 0 when one of
 * its factors was clamped.  g_j = dCS_j / d level j (j < M-1): gan_dssim's transposed-filter form with the maps of cs alone, centred,
 *   P = -(2 / B2) (mb - cs ma),   Q = 2 / B2,   R = -cs / B2;
 * g_{M-1} = dS_{M-1} / d level M-1 with gan_dssim's own P, Q, R.  G_j = k_j g_j + U(G_{j+1}), U the exact transpose of the pooling
 * (a pixel receives 0.25 of its parent's value once per time it is one of the parent's four taps), and
 *   dloss/da = -0.5 G_0 / (n c),
 * times grad_scale, times scale_state[0] when given.  The value of an image is its batch-1 value divided by n, rounded once.
 * grad_accumulate = 0: da = dtype_da(g);  1: da = dtype_da(float(da_old) + g), one fp32 addition, one rounding, as gan_edge_l1.
 * For a == b the loss and every da element are exactly 0.
 * Launches: M - 1 pooling launches, one statistics launch over the tiles of all levels (fp32 partial sums of cs and lum * cs per
 * (level, image, channel, 32 x 32 tile) into the workspace), one finalize launch (the partials added in a fixed order in double; MS,
 * per_image, the k_j and the loss word) - M + 1 launches for the loss alone - and, with da, one gradient launch per level from
 * the coarsest to level 0: 2 M + 1 in all (11 at M = 5).  Pooled levels, partials, coefficients and the gradients of the levels
 * above 0 live in the workspace as fp32.  No atomics, bit-identical from call to call, enqueue-only, capturable, allocates
 * nothing; each da element is written once by its owner thread. */
typedef struct GanMsssimDesc {
  uint32_t struct_size;
  int32_t dtype_a;             /* GAN_F32 | GAN_BF16 | GAN_F16: storage of a */
  int32_t dtype_b;             /* the same for b */
  GanTensor a;                 /* prediction: c = 1 or 3, own pitch; only the c real channels are read (pads may hold NaN) */
  GanTensor b;                 /* target: same n, h, w, c; own dtype and pitch */
  float loss_scale;
  int32_t loss_accumulate;     /* 0 | 1 */
  float* loss_out;             /* device: loss_out[0] (+)= loss_scale * loss, as gan_l1 */
  float grad_scale;
  int32_t dtype_da;            /* storage of da */
  GanTensor da;                /* ptr NULL: loss only.  Same n, h, w, c as a, own pitch; only the c real channels are (read and) written */
  void* workspace;             /* device: >= gan_msssim_workspace_bytes(n, h, w, c, scales), 4-byte aligned */
  size_t workspace_bytes;
  const float* scale_state;    /* fp16 loss scaling, as every loss entry point (the gradient only); NULL = none */
  int32_t scales;              /* M: 1 .. 5 */
  float power[5];              /* power[0 .. M-1], finite and >= 0; tf.image.ssim_multiscale: 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 */
  float* per_image;            /* device [n] or NULL: the score of every image (the call as a metric) */
  int32_t grad_accumulate;     /* 0: da = g;  1: da = round(float(da) + g) - a second term on a gradient another loss wrote */
} GanMsssimDesc;
/* 0 for a shape or a number of scales gan_msssim refuses */
size_t gan_msssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t scales);
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, n / h / w / c of a, b (and da) differ, n < 1, pitch < c,
 * loss_accumulate or grad_accumulate not 0 or 1, scales outside 1 .. 5, a power factor negative or not finite.  GAN_E_SHAPE: h or
 * w below 11 * 2^(scales - 1) or above 4096.  GAN_E_WORKSPACE: workspace too small.  All found before anything is launched: a
 * refused call writes nothing. */
int gan_msssim(const GanMsssimDesc* d, gan_stream_t stream);

/* ---- tiled inference: cut an image into overlapping network-sized tiles, blend the predictions back ------------------ */
/* Prediction at the source resolution (no counterpart in the reference, which resizes every image to img_size x img_size first,
 * pix2pix.py:43-52): an h x w image is cut into overlapping tile x tile pieces, the pieces go through one inference call as a
 * batch, and the outputs are blended back with weights that fall off towards the tile edges.
 * Geometry, per image axis of length L, with tile size S, overlap V and stride T = S - V:
 *     count n = 1 if L == S, else ceil((L - S) / T) + 1;   origin of tile k = min(k * T, L - S)
 * (the last tile is pulled back to end at the image edge: nothing is padded or extrapolated); the tiles of an image are
 * numbered row-major, t = ky * nx + kx.  Valid: L >= S, 0 <= V <= S / 2, S a multiple of 8 in [16, 1024], h and w <= 4096 -
 * then at most 3 tiles cover a pixel per axis, 9 in all.
 * Blend weight, per axis: the integer hat of the offset i inside the tile (0 <= i < S), hat(i) = min(i + 1, S - i) >= 1.  For
 * the image coordinate p, over the tiles k of the WHOLE grid that cover p, i_k = p - origin_k:
 *     a_k(p) = float(hat(i_k)) / float(sum_j hat(i_j))          one fp32 division of exactly representable integers
 * and for the pixel (py, px), channel ch:
 *     out = sum over ky ascending, inside it over kx ascending, of (a_ky(py) * a_kx(px)) * tile_value
 * Every product and every addition is rounded to fp32 on its own (nothing is contracted), the terms are added in that fixed
 * order, and the sum starts from 0.0f (accumulate = 0) or from the stored value (accumulate = 1).  A pixel that one tile covers
 * has weight exactly 1.0. */
/* Host only: the tile counts of an h x w image.  GAN_E_ARG: ny or nx NULL; GAN_E_SHAPE: the geometry is not valid (above). */
int gan_tile_grid(int32_t h, int32_t w, int32_t tile, int32_t overlap, int32_t* ny, int32_t* nx);

/* Tiles [t0, t0 + n) of one uint8 image, straight into a typed network input:
 *     dst[t - t0][r][x][ch] = dtype( lut[ src[(oy(t) + r) * src_pitch + (col0 + ox(t) + x) * c + ch] ] )
 * with (oy, ox) the origin of tile t.  Only the c real channels of a destination pixel are written: the pad channels of a wider
 * pitch keep what they hold, exactly as gan_pack leaves them.  Every source read is clamped to [0, src_bytes). */
typedef struct GanTileGatherDesc {
  uint32_t struct_size;
  int32_t dtype;               /* storage of dst: GAN_F32 | GAN_BF16 | GAN_F16 (round to nearest, as every conversion here) */
  const uint8_t* src;          /* device: first byte of the image's first row; c interleaved channels */
  int64_t src_bytes;           /* bytes readable from src */
  int32_t src_pitch;           /* bytes between consecutive source rows */
  int32_t col0;                /* first source column (pixels) of the part used: 0, or width / 2 for the right half of a pair */
  int32_t h, w;                /* size of the part used */
  int32_t c;                   /* 1 or 3 */
  int32_t tile, overlap;
  int32_t t0, n;               /* tiles of this launch */
  const float* lut;            /* device: 256 fp32 values, the normalised value of every byte (GanAugmentDesc.lut) */
  GanTensor dst;               /* n x tile x tile, c channels, own pitch; ptr aligned to its element size */
} GanTileGatherDesc;
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, dst not n x tile x tile x c, pitch < c, t0 / n outside the
 * grid, dst.ptr not element-aligned or lut not 4-byte aligned, col0 / src_pitch / the last row outside src_bytes.
 * GAN_E_SHAPE: as gan_tile_grid.  All found before anything is launched; enqueue-only. */
int gan_tile_gather_u8(const GanTileGatherDesc* d, gan_stream_t stream);

/* The same cut from a float image (no table): tiles [t0, t0 + n) of an fp32 / bf16 / fp16 image [h][src_pitch / c][c], for instance
 * the blended fp32 prediction of one generator as the input of the next (the cycle of a CycleGAN at the source resolution):
 *     dst[t - t0][r][x][ch] = dst_dtype( src[(oy(t) + r) * src_pitch + (col0 + ox(t) + x) * c + ch] )
 * Geometry and tile numbering are gan_tile_grid's.  src_dtype == dst_dtype copies the bits; an fp32 source is rounded to nearest
 * into a 16-bit destination, as every conversion here; no other pair is taken.  Only the c real channels of a destination pixel
 * are written; every source index is clamped to [0, src_elems). */
typedef struct GanTileGatherFDesc {
  uint32_t struct_size;
  int32_t src_dtype;           /* storage of src: GAN_F32 | GAN_BF16 | GAN_F16 */
  const void* src;             /* device: first element of the image's first row; c interleaved channels; element-aligned */
  int64_t src_elems;           /* elements readable from src */
  int32_t src_pitch;           /* elements between consecutive source rows */
  int32_t col0;                /* first source column (pixels) of the part used */
  int32_t h, w;                /* size of the part used */
  int32_t c;                   /* 1 or 3 */
  int32_t tile, overlap;
  int32_t t0, n;               /* tiles of this launch */
  int32_t dst_dtype;           /* storage of dst: src_dtype, or any of the three for an fp32 source */
  GanTensor dst;               /* n x tile x tile, c channels, own pitch; ptr aligned to its element size */
} GanTileGatherFDesc;
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype or dtype pair, c not 1 or 3, dst not n x tile x tile x c, pitch < c,
 * t0 / n outside the grid, src / dst.ptr not element-aligned, col0 / src_pitch / the last row outside src_elems.
 * GAN_E_SHAPE: as gan_tile_grid.  All found before anything is launched; enqueue-only, capturable. */
int gan_tile_gather(const GanTileGatherFDesc* d, gan_stream_t stream);

/* Tiles [t0, t0 + n) of a typed network output, added into the dense fp32 image [h][w][c] with the weights above.  One thread
 * owns an output pixel: it finds the tiles of this launch that cover it, adds them in ascending tile order and writes once -
 * no atomics, bit-identical from call to call.  A pixel that no tile of the launch covers keeps its value (accumulate = 1) or
 * becomes 0 (accumulate = 0).  The tiles of an image split over several launches in ascending order (accumulate = 0, then 1)
 * give the same bits as one launch. */
typedef struct GanTileBlendDesc {
  uint32_t struct_size;
  int32_t dtype;               /* storage of tiles */
  GanTensor tiles;             /* n x tile x tile, c channels, own pitch (the generator's output view) */
  float* image;                /* device: dense fp32 [h][w][c], 4-byte aligned */
  int32_t h, w, c;
  int32_t tile, overlap;
  int32_t t0, n;
  int32_t accumulate;          /* 0: start from 0.0f and overwrite; 1: start from the stored value */
} GanTileBlendDesc;
/* GAN_E_ARG: NULL pointer, wrong struct_size, bad dtype, c not 1 or 3, tiles not n x tile x tile x c, pitch < c, t0 / n outside
 * the grid, accumulate not 0 or 1, tiles.ptr not element-aligned or image not 4-byte aligned.  GAN_E_SHAPE: as gan_tile_grid. */
int gan_tile_blend(const GanTileBlendDesc* d, gan_stream_t stream);

/* Host utility (no GPU): CRC-32C of TensorFlow's TensorBundle checkpoint files (tf.train.Checkpoint /
 * CheckpointManager, pix2pix.py:400-403,419-420; cycle_gan.py:437-444,460-461).  crc = 0 to start; chainable. */
uint32_t gan_crc32c(uint32_t crc, const void* data, size_t n);
const char* gan_version(void);

/* ---- planner options -------------------------------------------------------------------------- */
/* The launch planners' tunable constants.  The library reads NO environment variable: these calls are the only way to
 * change them, and a change applies to the entry-point calls that follow it (each call plans for itself).  Unknown key:
 * GAN_E_ARG.  Keys (default): conv.big_tiles (1), conv.q128 (55), conv.q256n (80), conv.big_min_blocks (64),
 * conv.tall64 (1), conv.pingpong (1), conv.lean_epilogue (1), conv.tap_share (7: bit 0 = 256x128 tiles, bit 1 = 256x256 tiles on the tap-shared kernel, bit 2 = its table-driven form on the 256x128 tiles), conv.parity_patch (1), conv.parity_patch_max_n (64),
 * conv.parity_patch_min_blocks (192), conv.split_target (256), conv.split_target_skinny (1024),
 * conv.split_target_big (256), conv.split_target_256 (128), conv.split_min_ktiles (4), conv.split_max (64), conv.bwd_fuse_tile (1: the fused backward
 * epilogue rides on every tile epilogue; 0 never, 2 not on 64-column tiles, 3 on 64-column tiles only), conv.thin (7: bit 0
 * streaming kernels for the <= 8-channel layers, bit 1 thin-N, bit 2 thin-K), conv.norm_fuse (1), conv.stack (0: the callers in gan_amd/ merge eligible runs into layer stacks only when set), conv.stack_blocks (256), conv.thin_fused (1), wgrad.tile256 (0), wgrad.pingpong (1), wgrad.row_table (1),
 * wgrad.pingpong_min_rows (0 = automatic), wgrad.pingpong_128 (1), wgrad.pingpong_min_gflop (30),
 * wgrad.split_target (512), wgrad.fold_split_target (512), wgrad.reduce_adam (1),
 * wgrad.reduce_adam_min_params (1048576: smaller kernels keep the flat slab reduce and the caller's multi-tensor Adam pass),
 * conv.reduce_stats_rg (16: the slab reduce of a split-K launch that also emits the statistics partials walks up to this many row groups
 * per workgroup, one chunk each - keeps the chunk count of a 4,096-row 512-channel layer under ~512 so that the fused path is taken),
 * conv.own_max_rows (16) / conv.own_max_kb (192): a norm_fuse layer of at most this many GEMM rows per parity (<= 64; 0: never) whose
 * live taps x (8 weight rows + its rows) stay under this many KB per workgroup runs on the column-owner kernel (csrc/conv_own.hip)
 * instead of split-K GEMM + finishing slab reduce - same products, another fixed summation order,
 * wgrad.dead_taps (1: a fused-Adam wgrad launch skips the taps that never meet the map at its shape - 12 of 16 for a 2x2 -> 1x1
 * layer - where their moments are zero: the update is the identity there), diag.launch_log (0: see gan_launch_log below). */
int gan_set_option(const char* key, int32_t value);
int gan_get_option(const char* key, int32_t* value);
/* Diagnostic launch log (profiling tools only; no counterpart in the reference, whose only timing is time.time() per epoch,
 * pix2pix.py:261,319).  gan_set_option("diag.launch_log", 1) clears the log and starts recording the kernel symbol of EVERY
 * launch the entry points make, in enqueue order (0 stops).  gan_launch_log() copies the mangled names, newline-separated, into
 * buf (at most cap bytes, NUL-terminated) and returns the bytes the whole log needs.  tools/class_profile.py joins it with a
 * rocprofv3 --kernel-trace of the replayed step: per-launch class label + algorithmic FLOPs beside the measured duration. */
size_t gan_launch_log(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
