/*
 * savfi_hip.h -- C ABI of libsavfi_hip.so, the MI355X (gfx950) kernels behind the
 * MAML inner-loop adaptation path of scene-adaptive video frame interpolation.
 *
 * This header is the drop-in boundary.  Each entry point replaces one piece of the
 * reference's hot path (file:line are relative to the reference checkout):
 *
 *   savfi_sepconv_fwd_f32      kernel_Sepconv_updateOutput            sepconv/sepconv_op/sepconv.py:5-30, launch :280-291
 *   savfi_sepconv_bwd_f32      kernel_Sepconv_updateGradVertical      sepconv/sepconv_op/sepconv.py:138-163, launch :343-356
 *                              kernel_Sepconv_updateGradHorizontal    sepconv/sepconv_op/sepconv.py:165-190, launch :358-371
 *                              kernel_Sepconv_updateGradInput         sepconv/sepconv_op/sepconv.py:32-63,  launch :328-341
 *   savfi_voxelwarp_fwd_f32    flow/mask split + meshgrid + 2x grid_sample + blend
 *   savfi_voxelwarp_bwd_f32                                          voxelflow/core/models/voxel_flow.py:471-509, :9-17
 *   savfi_avgpool2x2_fwd/bwd_f32  2x2 average pooling                 sepconv/model.py:176-187, rrin/unet.py:146, superslomo/model.py:66
 *   savfi_flowwarp_fwd/bwd_f32 pixel-flow backward warp              superslomo/model.py:231-307, rrin/model.py:8-20
 *   savfi_pixel_unshuffle_f32  pixel_shuffle(scale<1)                 model_utils.py:202-217 (else branch)
 *   savfi_pixel_shuffle_f32    pixel_shuffle(scale>=1)                model_utils.py:202-217 (if branch)
 *   savfi_mt_update_f32        LSLR / Meta-SGD update_sgd/adam/adamax inner_loop_optimizers.py:136-244, :324-425
 *   savfi_mt_update_bwd_f32    (autograd of the above w.r.t. the learning rates)
 *   savfi_mt_mean_f32          per-tensor mean of grads (L2F embedding) meta_learning_system.py:249-253
 *   savfi_mt_scale_f32         gamma_i * w_i (L2F attenuation)        meta_learning_system.py:267-268
 *   savfi_l1_mse_f32           nn.L1Loss / nn.MSELoss                 loss.py:287-290
 *   savfi_ssim_loss_f32        pytorch_msssim.SSIM as Loss constructs it, forward and gradient   loss.py:294, pytorch_msssim/__init__.py:7-131
 *   savfi_psnr_ssim_f32        utils.quantize + calc_psnr's squared error + ssim(val_range=255), `rows` image pairs per call   utils.py:171-204, pytorch_msssim/__init__.py:19-75
 *   savfi_msssim_f32 / _bwd_f32  pytorch_msssim.msssim as implemented (five levels, per-level range rule), forward and gradient   pytorch_msssim/__init__.py:78-104
 *   savfi_upsample2x_fwd/bwd_f32  bilinear x2 up-sampling                 sepconv/model.py:191,213-234; voxel_flow.py:400-414
 *   savfi_upsample2x_window_fwd/bwd_f32  the same map on a window (SepConv Subnets on the frame area)  sepconv/model.py:309-349
 *   savfi_bias_act_fwd/bwd_f32 conv bias add + (Leaky)ReLU and their backward + bias gradient
 *                                                                     sepconv/model.py:172-194, model_utils.py:957-990
 *   savfi_conv3x3_f32          F.conv2d 3x3 / stride 1 (+ bias, activation) and its data gradient
 *   savfi_conv3x3_wgrad_f32    its weight gradient                    model_utils.py:308-366 (MetaConv2dLayer.forward -> F.conv2d)
 *   savfi_conv3x3_tasks_f32, savfi_conv3x3_wgrad_tasks_f32   the same for T tasks with their own fast weights in ONE launch
 *   savfi_conv3x3_filters_f32, savfi_conv3x3_tasks_pre_f32   filter transforms of forward + data gradient in one launch / convolution on a transformed filter
 *                              (the sequential task loop meta_learning_system.py:366 run in lockstep)
 *   savfi_convk_filters_f32, savfi_convk_tasks_pre_f32, savfi_convk_wgrad_tasks_f32   F.conv2d K x K (K = 3, 5, 7) / stride 1 and its data gradient as a direct
 *                              implicit GEMM on the bf16 matrix cores from error-free 3-way operand splits (fp32-equivalent)
 *                                                                     voxelflow/core/models/voxel_flow.py:357-470 (5x5 layers),
 *                                                                     superslomo/model.py:547-646 (7x7 / 5x5), model_utils.py:308-366
 *   savfi_ca_pool/mlp_fwd/mlp_bwd/apply_f32   channel attention + residual of CAIN's RCAB   model_utils.py:931-953, :957-990
 *   savfi_frames_u8_to_f32     HWC uint8 frames -> normalised fp32 NCHW  data/vimeo_septuplet.py:68-80, data/video.py:44-51
 *   savfi_frames_f32_to_u8     unit-range fp32 NCHW -> quantised uint8 NHWC (what save_image writes)   utils.py:171-172, :276-285
 *   savfi_filterinterp_fwd/bwd_f32   DAIN's adaptive warping layer (per-pixel 4x4 filter at the flow-displaced position)
 *   savfi_filterinterp_fwd_slice_f32 the same forward written into a channel slice of a wider tensor (MetaDAIN's rectify input)
 *                                                                     dain/my_package/FilterInterpolation/filterinterpolation_cuda_kernel.cu:29-460
 *   savfi_depthflowproj_fwd/bwd_f32  DAIN's depth-aware flow projection (scatter, average, hole fill)
 *                                                                     dain/my_package/DepthFlowProjection/depthflowprojection_cuda_kernel.cu:29-341
 *   savfi_correlation_fwd/bwd_f32    PWC-Net's cost-volume correlation (md = 4), LeakyReLU fused   dain/PWCNet/correlation_package_pytorch1_0/
 *                                                                     correlation_cuda_kernel.cu:73-340
 *   savfi_pwcwarp_fwd_f32            PWC-Net's warp: bilinear sample (align_corners) times the thresholded sample of ones
 *                                                                     dain/PWCNet/PWCNet.py:158-198
 *   savfi_bn_stats/bn_apply_relu/bn_running_update_f32   train-mode BatchNorm2d + ReLU of DAIN's depth hourglass, per task
 *                                                                     dain/MegaDepth/pytorch_DIW_scratch.py:31-760
 *   savfi_maxpool2x2/upnearest2x_add/add_relu_f32        the pooling, upsample + skip sum and residual tail of DAIN's sub-networks
 *                                                                     dain/networks/DAIN.py:692-824, dain/Resblock/BasicBlock.py:97-149
 *   savfi_charbonnier_f32 / _bwd_f32 DAIN's Charbonnier loss         dain/loss_function.py:14-16
 *   savfi_*_workspace_floats / savfi_bias_act_scratch_floats: sizes of the caller-owned scratch buffers (return int64_t)
 *
 * Conventions (all functions):
 *   - extern "C", return int: 0 = ok; >0 = hipError_t reported by the launch;
 *     <0 = argument error (SAVFI_E_*).  No exceptions cross the boundary.
 *   - every pointer is a DEVICE pointer to a contiguous fp32 NCHW buffer owned by the
 *     caller, unless the parameter is documented as a host array.  The library never
 *     allocates device memory, never synchronises, and is re-entrant.
 *   - `stream` is a hipStream_t passed as void* (the caller passes
 *     torch.cuda.current_stream().cuda_stream); launches are asynchronous on it.
 */
#ifndef SAVFI_HIP_H_
#define SAVFI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Counts INCOMPATIBLE changes: an entry removed or its arguments or meaning changed.  Entries that are only added leave it alone
 * (a binding written for the older header still works).  Added under 24: savfi_correlation_fwd_f32, savfi_correlation_bwd_f32,
 * savfi_pwcwarp_fwd_f32; then, for DAIN's frozen front and rectify net, savfi_bn_stats_scratch_floats, savfi_bn_stats_f32,
 * savfi_bn_apply_relu_f32, savfi_bn_running_update_f32, savfi_maxpool2x2_f32, savfi_upnearest2x_add_f32, savfi_add_relu_f32,
 * savfi_charbonnier_f32, savfi_charbonnier_bwd_f32; then savfi_conv3x3_f4_launched_workgroups, savfi_conv3x3_debug_f4_block_decode,
 * savfi_conv3x3_tasks_pre_pool_f32; then savfi_filterinterp_fwd_slice_f32; then, for multi-scale
 * SSIM, savfi_msssim_scratch_bytes, savfi_msssim_f32, savfi_msssim_bwd_f32; then, for SepConv's second-order terms,
 * savfi_sepconv_bwd2_f32; then savfi_upsample2x_bwd_form; then, for the Laplacian-pyramid loss term, savfi_laploss_scratch_bytes,
 * savfi_laploss_f32, savfi_laploss_bwd_f32; then, for the census loss term, savfi_census_scratch_bytes, savfi_census_f32,
 * savfi_census_bwd_f32; then, for the second-order terms of the two warps, savfi_voxelwarp_bwd2_f32, savfi_flowwarp_bwd2_f32; then, with
 * the one SepConv route, savfi_sepconv_route, savfi_sepconv_debug_span_bytes; then, for the deep layers' small maps,
 * savfi_convk_wgrad3_small_plan, savfi_convk_wgrad3_small_route, savfi_convk_wgrad3_small_workspace_floats,
 * savfi_convk_wgrad3_small_tasks_f32, savfi_convk_wgrad3_small_tasks_bias_f32; then, for the AdaCoF plugin's deformable-tap op,
 * savfi_adacof_fwd_f32, savfi_adacof_bwd_f32; then, for softmax splatting (forward warping), savfi_softsplat_scratch_bytes,
 * savfi_softsplat_fwd_f32, savfi_softsplat_bwd_f32. */
#define SAVFI_ABI_VERSION 24

#define SAVFI_OK            0
#define SAVFI_E_NULL       (-1)  /* a required pointer is NULL                          */
#define SAVFI_E_SHAPE      (-2)  /* a dimension is <= 0 or inconsistent                  */
#define SAVFI_E_UNSUPPORTED (-3) /* e.g. scale factor / rule id not implemented          */
#define SAVFI_E_TOOBIG     (-4)  /* index arithmetic would overflow 32-bit element index */

/* ABI version of the loaded library (== SAVFI_ABI_VERSION it was built against). */
int savfi_version(void);

/* ------------------------------------------------------------------------------------
 * Separable local convolution (SepConv), K taps per axis (K = 51 in the model).
 *   in  [B, C, Ho+K-1, Wo+K-1]   v, h [B, K, Ho, Wo]   out [B, C, Ho, Wo]
 *   out[b,c,y,x] = sum_{fy<K} sum_{fx<K} in[b,c,y+fy,x+fx] * v[b,fy,y,x] * h[b,fx,y,x]
 * ---------------------------------------------------------------------------------- */
int savfi_sepconv_fwd_f32(const float* in, const float* v, const float* h, float* out,
                          int B, int C, int Ho, int Wo, int K, void* stream);

/* Gradients of the above.  Any of gI / gV / gH may be NULL (= not needed, like
 * needs_input_grad in sepconv.py:319-321).  gI is the mathematically exact adjoint
 * (the reference's kernel has an off-by-one bounds test, sepconv.py:51,54).
 *   gO [B,C,Ho,Wo]  gI [B,C,Ho+K-1,Wo+K-1]  gV, gH [B,K,Ho,Wo]
 * Outputs are fully overwritten (no pre-zeroing needed). */
int savfi_sepconv_bwd_f32(const float* in, const float* v, const float* h, const float* gO,
                          float* gI, float* gV, float* gH,
                          int B, int C, int Ho, int Wo, int K, void* stream);

/* The backward of the FILTER gradients above (second order; csrc/sepconv_bwd2.hip).  With gV, gH = the filter gradients of the op for the
 * upstream gO, cotangents ggV of gV and ggH of gH (each [B,K,Ho,Wo]) and frames that carry no gradient, sep(.) the forward:
 *   d_gO [B,C,Ho,Wo] = sep(in, ggV, h) + sep(in, v, ggH)
 *   dV   [B,K,Ho,Wo] = the gV formula with h <- ggH         dH [B,K,Ho,Wo] = the gH formula with v <- ggV
 * ggV or ggH may be NULL (= zero), not both.  Each of d_gO / dV / dH may be NULL (= not wanted), not all three.  dV needs ggH and dH
 * needs ggV: asking for one whose cotangent is NULL is SAVFI_E_NULL (it would be all zero; the caller returns no gradient instead).
 * fp32 operands and accumulators; every requested element is written exactly once from a sequential sum: no atomics, no pre-zeroing,
 * no host read -- capturable and bit-reproducible.  One launch.  Any K, C; K = 51, C = 3 runs on the fp32 matrix cores.
 * Errors, checked in this order before any launch: SAVFI_E_NULL (above); SAVFI_E_SHAPE (a dimension <= 0); SAVFI_E_UNSUPPORTED (an
 * output pointer equal to an operand or to another output, or a pointer that is not 4-byte aligned); SAVFI_E_TOOBIG (the limits of
 * savfi_sepconv_bwd_f32: B*K, B*C, Ho+K-1 <= 65535, Wo+K-1 < 2^31, tensors below 2^40 elements). */
int savfi_sepconv_bwd2_f32(const float* in, const float* v, const float* h, const float* gO,
                           const float* ggV, const float* ggH,
                           float* d_gO, float* dV, float* dH,
                           int B, int C, int Ho, int Wo, int K, void* stream);

/* The same op on tap tensors that are slices of ONE interleaved buffer: sample b of v / h (and of gV / gH) starts tap_bstride planes of
 * Ho * Wo floats after sample b - 1 (tap_bstride = K: the contiguous layout of the two entry points above).  The package's SepConv plugin
 * evaluates the reference's four Subnets (sepconv/model.py:183-194, :239-242, :346-347) as one task-batched launch per layer; their taps are
 * a [B * 4, K, Ho, Wo] tensor (sample 4 b + s = sub-network s) that the two local convolutions read -- and their filter gradients write --
 * in place with tap_bstride = 4 * K.  K = 51, C = 3, Wo % 4 == 0, every tensor below 2^31 bytes; SAVFI_E_UNSUPPORTED otherwise (the
 * caller copies the slices and uses the contiguous entry points).  No gI (frames carry no gradient on this path). */
/* 1 when the strided / frames8 / pair entry points take the problem in this library (shapes, sizes AND the switches of a variant build
 * that make them return SAVFI_E_UNSUPPORTED), 0 otherwise: what a caller asks before it chooses the interleaved tap tensor.  They take
 * what savfi_sepconv_route (below) sends to the wave-specialised kernels for want = 3 in ONE launch (chunk == B), with the strided tap
 * buffer inside the span too; they do not cut a batch into chunks. */
int savfi_sepconv_taps_strided_supported(int B, int C, int Ho, int Wo, int K, int tap_bstride);
int savfi_sepconv_fwd_taps_strided_f32(const float* in, const float* v, const float* h, float* out, int B, int C, int Ho, int Wo, int K,
                                       int tap_bstride, void* stream);
int savfi_sepconv_bwd_taps_strided_f32(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH, int B,
                                       int C, int Ho, int Wo, int K, int tap_bstride, void* stream);

/* Frames of 8-bit images.  The reference hands the op decoded PNG frames: ToTensor's k / 255 with k = 0..255 (data/vimeo_septuplet.py:24-36;
 * sepconv/model.py:346-347 only replication-pads them).  255 * in is then an integer that one bf16 holds exactly, and an fp32 product
 * in * tap costs three exact bf16 products (k times the tap's three bf16 pieces) instead of six; the sum is scaled by 1/255 once.
 *   savfi_frames8_classify_f32   x [n] floats -> cls [SAVFI_FRAMES8_WORDS] words (device, 16-byte aligned, need not be initialised):
 *                                word i != 0 = classifier workgroup i met an element that is not fl32(k / 255) to within 2 ulp
 *   savfi_sepconv_{fwd,bwd}_frames8_f32   the two strided entry points above with the words of `in` as an extra argument.  BOTH kernel
 *                                variants are launched and the words select one ON THE DEVICE (no host round trip, graph-capture safe):
 *                                all words zero -> the three-product kernel, otherwise the six-product kernel of the entry points above.
 *                                Same results to fp32 rounding for frames that qualify, identical results for frames that do not.
 * tap_bstride = K for contiguous tap tensors.  K = 51, C = 3, Wo % 4 == 0; SAVFI_E_UNSUPPORTED otherwise (use the entry points above).
 * taps_unit16 != 0: v and h are UNIT-MAJOR -- a sample is [Ho][Wo / 16][K][16] instead of [K][Ho][Wo], the layout
 *   savfi_conv3x3_tasks_pre_unit16_f32 writes (Wo % 16 == 0): the 51 taps of 16 neighbouring pixels are one contiguous run of
 *   51 x 64 bytes instead of 64-byte pieces of 51 planes.  The sample stride (tap_bstride planes of Ho * Wo floats) is unchanged, and
 *   gV / gH are written [K][Ho][Wo] (what the producing convolution's gradient kernels read) unless bit 1 is set as well (taps_unit16 = 3,
 *   backward only): then gV / gH are unit-major too -- for a producer whose data gradient reads that layout (savfi_conv3x3_dgrad_in_unit16_f32)
 *   and whose weights need no gradient in this pass. */
#define SAVFI_FRAMES8_WORDS 256
int savfi_frames8_classify_f32(const float* x, int64_t n, unsigned* cls, void* stream);
int savfi_sepconv_fwd_frames8_f32(const float* in, const float* v, const float* h, float* out, const unsigned* cls, int B, int C, int Ho,
                                  int Wo, int K, int tap_bstride, int taps_unit16, void* stream);
int savfi_sepconv_bwd_frames8_f32(const float* in, const float* v, const float* h, const float* gO, float* gV, float* gH,
                                  const unsigned* cls, int B, int C, int Ho, int Wo, int K, int tap_bstride, int taps_unit16, void* stream);

/* The two filter-gradient calls of an interleaved tap tensor as ONE launch (the plugin's tail: sepconv/model.py:346-347 evaluates
 * FunctionSepconv twice, on frame 0 with sub-networks 0 / 1 and on frame 1 with sub-networks 2 / 3, and adds the results -- their backward
 * passes share the cotangent gO).  taps, gtaps [4 B][K][Ho][Wo] (sample 4 b + s = sub-network s: v0, h0, v1, h1); in0, in1 the frames with
 * their own classifier words.  The three-product kernel runs when BOTH frames qualify.  A launch of these kernels has a fixed cost of about
 * 24 us at 256 x 448, so one launch over 2 B samples is faster than two over B; the results are the same bit for bit.  taps_unit16 as above.
 * The forward of the pair the same way: out [B][2][C][Ho][Wo] holds the two local convolutions of every sample, the caller adds them. */
int savfi_sepconv_fwd_pair_frames8_f32(const float* in0, const float* in1, const float* taps, float* out /* [B][2][C][Ho][Wo] */,
                                       const unsigned* cls0, const unsigned* cls1, int B, int C, int Ho, int Wo, int K, int taps_unit16,
                                       void* stream);
int savfi_sepconv_bwd_pair_frames8_f32(const float* in0, const float* in1, const float* taps, const float* gO, float* gtaps,
                                       const unsigned* cls0, const unsigned* cls1, int B, int C, int Ho, int Wo, int K, int taps_unit16,
                                       void* stream);

/* Diagnostic of the wave-specialised filter-gradient kernel (csrc/sepconv_ws.hip): number of bounded in-kernel waits that
 * gave up since the library was loaded on the current device.  0 on a healthy build; > 0 means a launch's numbers are wrong
 * (the kernel never hangs).  Synchronises with the device.  -1: the counter could not be read. */
int savfi_sepconv_ws_errors(void);
/* The same count WITHOUT a device synchronisation.  savfi_sepconv_ws_watch() -- once per device, outside a stream capture -- maps one host
 * word into the device; a wait that gives up also adds to that word (system-scope atomic), which the host sees at the latest when the
 * launch has completed.  savfi_sepconv_ws_errors_peek() reads the word: the caller checks it wherever it has synchronised anyway (the
 * package: after reading an iteration's loss, meta_learning_system.py) and refuses the iteration's numbers when it is non-zero.
 * -1: not armed on this device. */
int savfi_sepconv_ws_watch(void);
int savfi_sepconv_ws_errors_peek(void);
/* Clears the current device's mapped word and returns the count it held (-1: not armed): for a caller that has handled the reported
 * time-out (the product drops the meta-iteration BEFORE its outer optimizer step and raises) and goes on. */
int savfi_sepconv_ws_errors_reset(void);
/* Test hook: the spin limit of the kernels' bounded waits (default 1 << 19 spins of s_sleep 2).  A NEGATIVE limit makes every wait that does
 * not find its flag at once give up -- tests/ provoke the error path with it.  *previous (may be NULL) receives the old limit; launches issued afterwards use the new one. */
int savfi_sepconv_ws_debug_spin_limit(int limit, int* previous);

/* The work partition of the persistent SepConv kernels (K = 51, C = 3).  They launch at most one workgroup per CU; the phases of all
 * strips in strip-major order (position g: strip g / nph, phase g % nph; strip s: sample s / ncol, strip s % ncol of the sample) are cut
 * into one piece per workgroup, and a piece that crosses into the next strip starts a new run (a new LDS window) there.
 *   kind SAVFI_SEPCONV_PARTITION_WS    the wave-specialised kernels (csrc/sepconv_ws.hip: Wo % 4 == 0, the strided / frames8 / pair entry
 *                                      points; a pair launch over B samples is B' = 2 B here): phases of 4 rows, strips of 32 columns
 *        SAVFI_SEPCONV_PARTITION_X6    one program per wave (csrc/sepconv_x6.hip: other widths): phases of 4 rows, strips of 32 columns
 *        SAVFI_SEPCONV_PARTITION_FP32  the fp32 kernel of savfi_sepconv_bwd_f32 with one of gV / gH NULL: phases of 2 rows, strips of 64
 * savfi_sepconv_partition answers with the host code the launches use and the functions the kernels evaluate: [*g0, *g1) is the piece of
 * workgroup `block` in a launch planned for `cus` CUs (cus <= 0: the count launches plan for now).  Returns the grid size (<= cus), or
 * SAVFI_E_NULL / SAVFI_E_SHAPE (a dimension <= 0, block outside the grid) / SAVFI_E_TOOBIG (the persistent kernels do not take the
 * problem) / SAVFI_E_UNSUPPORTED (kind).  Needs no device. */
#define SAVFI_SEPCONV_PARTITION_WS   0
#define SAVFI_SEPCONV_PARTITION_X6   1
#define SAVFI_SEPCONV_PARTITION_FP32 2
int savfi_sepconv_partition(int kind, int B, int Ho, int Wo, int cus, int block, int* g0, int* g1);
/* The route of savfi_sepconv_fwd_f32 / savfi_sepconv_bwd_f32: which kernel a call runs, and on how many consecutive samples per launch.
 *   want   0 = forward, 1 = gV only, 2 = gH only, 3 = gV and gH (gI is always one direct launch over the whole batch)
 *   chunk  the largest Bc <= B for which both Bc * 51 * Ho * Wo * 4 and Bc * 3 * (Ho + 50) * (Wo + 50) * 4 are below the span of 2^31
 *          bytes (the persistent kernels address each tensor through one buffer descriptor); 0 if not even one sample fits
 *   K == 51, C == 3 and chunk > 0:  want 0 or 3 -> SAVFI_SEPCONV_PARTITION_WS if Wo % 4 == 0, else SAVFI_SEPCONV_PARTITION_X6
 *                                   want 1 or 2 -> SAVFI_SEPCONV_PARTITION_FP32
 *   anything else:                  SAVFI_SEPCONV_ROUTE_DIRECT (one thread per output element), reported with chunk = B
 * With chunk < B the entry point launches the kernel once per run of `chunk` consecutive samples (the last run shorter): ordinary
 * launches on the caller's stream, capturable; every sample's bits are those of a call with that sample alone.
 * Variant builds: -DSAVFI_SEPCONV_NO_MFMA always DIRECT; _NO_WS: X6 where WS stands above (_NO_WS_FWD: for want == 0 only); _F32_MFMA:
 * FP32 for every want != 0.
 * Returns the kernel, or SAVFI_E_SHAPE (want outside 0..3, a dimension <= 0) / SAVFI_E_TOOBIG (the limits of savfi_sepconv_fwd_f32);
 * *chunk (may be NULL) receives the chunk.  Needs no device.  savfi_sepconv_partition answers SAVFI_E_TOOBIG exactly where chunk < B. */
#define SAVFI_SEPCONV_ROUTE_DIRECT 3
int savfi_sepconv_route(int want, int B, int C, int Ho, int Wo, int K, int* chunk);
/* Test hook: the CU count that the launches of those kernels plan for.  0 restores the device's count; other values are clamped to
 * [1, device count].  Host side only -- fewer workgroups that take more phases each is an ordinary launch (there is no dependency
 * between workgroups) -- so tests/ can drive every state of the partition on any device.  *previous (may be NULL) receives the old
 * setting (0 = the device's count); launches issued afterwards use the new one. */
int savfi_sepconv_debug_cus(int cus, int* previous);
/* Test hook: the span (bytes) that the route above holds the tensors of one persistent launch below.  0 restores 2^31; other values are
 * clamped to [1, 2^31].  Host state only -- a smaller span means more, smaller launches; nothing in a kernel reads it -- so tests/ can
 * drive the chunk loop on small tensors.  *previous (may be NULL) receives the old span; calls issued afterwards use the new one. */
int savfi_sepconv_debug_span_bytes(int64_t bytes, int64_t* previous);

/* ------------------------------------------------------------------------------------
 * VoxelFlow warp + blend (syn_type 'inter').
 *   frames [B,6,H,W] (I0 = ch 0..2, I1 = ch 3..5), x3 [B,3,H,W] = tanh output
 *   flow = 0.5*x3[:,0:2] (normalised units), mask = 0.5*(1+x3[:,2])
 *   out[b,c] = mask * bilinear(I0, grid - flow) + (1-mask) * bilinear(I1, grid + flow)
 *   with grid = linspace(-1,1), align_corners=True, padding_mode='border'.
 * bwd: g_x3 [B,3,H,W] always written; g_frames [B,6,H,W] may be NULL (frames are data).
 *      When g_frames != NULL it must be zero-filled by the caller (scatter-add).
 * ---------------------------------------------------------------------------------- */
int savfi_voxelwarp_fwd_f32(const float* frames, const float* x3, float* out,
                            int B, int H, int W, void* stream);
int savfi_voxelwarp_bwd_f32(const float* frames, const float* x3, const float* gO,
                            float* g_x3, float* g_frames,
                            int B, int H, int W, void* stream);
/* The backward of g_x3 above (second order, frames constant).  v [B,3,H,W] is the cotangent of g_x3.  Per pixel, with A. / B. the
 * coordinate slopes of tap a (I0) / tap b (I1) -- (size-1)/2, 0 where the coordinate is clipped --, DX / DY the derivatives of a tap's
 * sample by its source position and X the mixed difference of its four corners (both zero across a dropped upper corner):
 *   d_gO [B,3,H,W] = 0.5 (v0 ((1-m) Bx DXb - m Ax DXa) + v1 ((1-m) By DYb - m Ay DYa) + v2 (o1 - o2))
 *   d_x3 [B,3,H,W] = H v,  H00 = H11 = H22 = 0,  H01 = 0.25 sum_c gO (m Ax Ay Xa + (1-m) Bx By Xb),
 *                    H02 = -0.25 sum_c gO (Ax DXa + Bx DXb),  H12 = -0.25 sum_c gO (Ay DYa + By DYb)
 * Either output may be NULL (= not computed, not written), not both.  One launch, a gather: no atomics, no pre-zeroing, every element
 * written once -- capturable and bit-reproducible.  Errors as savfi_voxelwarp_bwd_f32: SAVFI_E_NULL, SAVFI_E_SHAPE. */
int savfi_voxelwarp_bwd2_f32(const float* frames, const float* x3, const float* gO, const float* v,
                             float* d_gO, float* d_x3, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * 2x2 / stride 2 average pooling of `planes` = N*C maps [H,W] -> [H/2,W/2] (floor): torch.nn.AvgPool2d(2, 2)
 * sepconv/model.py:176-187, F.avg_pool2d(x, 2) rrin/unet.py:146, superslomo/model.py:66.
 *   fwd: out[y][x] = (in[2y][2x] + in[2y][2x+1] + in[2y+1][2x] + in[2y+1][2x+1]) / 4
 *   bwd: gin [planes,H,W] fully written: gout[y/2][x/2] / 4, zero in an odd last row / column
 * ---------------------------------------------------------------------------------- */
int savfi_avgpool2x2_fwd_f32(const float* in, float* out, int64_t planes, int H, int W, void* stream);
int savfi_avgpool2x2_bwd_f32(const float* gout, float* gin, int64_t planes, int H, int W, void* stream);
/* the adjoint of "pool AND keep": an activated map y [planes,H,W] feeds the pooling and, unchanged, a skip connection (an encoder block
 * of sepconv/model.py:176-187 + the decoder's `tensorUpsample + tensorConv`); gout [planes,H/2,W/2] and gskip [planes,H,W] are the two
 * consumers' cotangents (either may be NULL), and the (leaky) ReLU derivative of y's producer is applied in the same pass (y NULL: none):
 *   gin = (gout[y/2][x/2] / 4 + gskip) * (y > 0 ? 1 : slope)
 * -- what autograd runs as the pooling's adjoint, an accumulation and ReLU's backward: three element-wise passes. */
int savfi_avgpool2x2_bwd_fused_f32(const float* gout, const float* gskip, const float* y, float slope, float* gin, int64_t planes, int H, int W,
                                   void* stream);

/* ------------------------------------------------------------------------------------
 * Backward warping by a pixel-unit flow (SuperSloMo backWarp superslomo/model.py:231-307, RRIN warp
 * rrin/model.py:8-20: meshgrid + 2*(x/W-0.5) normalisation + F.grid_sample(bilinear, zeros, align_corners=False)).
 *   img [N,C,H,W], flow [N,2,H,W] (u, v in pixels) -> out [N,C,H,W]
 *   out[n,c,y,x] = bilinear(img[n,c]; x + u - 0.5, y + v - 0.5), corners outside the image count as zero
 *   (the half-pixel offset is what the reference's normalisation amounts to under align_corners=False).
 * bwd: gflow [N,2,H,W] = dL/d(u,v), fully written (a gather: deterministic).  No image gradient: the warped
 *      images are network inputs on this path.
 * ---------------------------------------------------------------------------------- */
int savfi_flowwarp_fwd_f32(const float* img, const float* flow, float* out, int N, int C, int H, int W, void* stream);
int savfi_flowwarp_bwd_f32(const float* img, const float* flow, const float* gout, float* gflow,
                           int N, int C, int H, int W, void* stream);
/* The backward of the flow gradient above (second order, img constant).  v [N,2,H,W] = (vu, vv) is the cotangent of gflow; with
 * Dx_c / Dy_c the derivatives of out[c] by the source position, X_c = (se - sw) - (ne - nw) the mixed difference of the cell's corners
 * (corners outside the image count as zero) and sx = (W/2)*(2/W), sy = (H/2)*(2/H) in fp32 as the first order applies them:
 *   d_gout [N,C,H,W] = vu sx Dx_c + vv sy Dy_c
 *   d_flow [N,2,H,W] = (vv, vu) sx sy sum_c gout_c X_c            (the diagonal of the per-pixel Hessian is zero inside a cell)
 * A pixel whose cell has no corner inside the image (far outside, NaN / inf flow) gets zeros in both.  Either output may be NULL (= not
 * computed, not written), not both.  One launch, a gather: no atomics, no pre-zeroing, every element written once -- capturable and
 * bit-reproducible.  Errors as savfi_flowwarp_bwd_f32: SAVFI_E_NULL, SAVFI_E_SHAPE, SAVFI_E_TOOBIG. */
int savfi_flowwarp_bwd2_f32(const float* img, const float* flow, const float* gout, const float* v,
                            float* d_gout, float* d_flow, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * Pixel (un)shuffle with the reference's channel order.
 *   unshuffle: in [B,C,H,W] -> out [B,C*r*r,H/r,W/r], out ch = c*r*r + i*r + j
 *              out[b, c*r*r+i*r+j, y, x] = in[b, c, y*r+i, x*r+j]
 *   shuffle:   in [B,C*r*r,H,W] -> out [B,C,H*r,W*r]   (exact inverse)
 * Dimensions passed are those of `in`.  Each is the other's autograd adjoint.
 * ---------------------------------------------------------------------------------- */
int savfi_pixel_unshuffle_f32(const float* in, float* out, int B, int C, int H, int W, int r, void* stream);
int savfi_pixel_shuffle_f32(const float* in, float* out, int B, int C, int H, int W, int r, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused multi-tensor inner-loop update (one launch per <= SAVFI_MT_MAX_TENSORS tensors;
 * the library chunks internally).  Host arrays of device pointers, length n.
 *
 *   rule: SAVFI_RULE_SGD      out = w - lr * g
 *         SAVFI_RULE_ADAM     m = b1*m + (1-b1)*g ; s = b2*s + (1-b2)*g*g   (m, s updated IN PLACE)
 *                             out = w - (lr/bc1) * m / (sqrt(s)/sqrt(bc2) + eps)
 *         SAVFI_RULE_ADAMAX_LSLR   m = b1*m + (1-b1)*g (in place) ; out = w - (lr/bc1) * m / (|g| + eps)
 *         SAVFI_RULE_ADAMAX_MSGD   out = w - (lr/bc1) * ((1-b1)*g) / (|g| + eps)   (state untouched)
 *       (the two Adamax forms are the reference's as-implemented arithmetic,
 *        inner_loop_optimizers.py:201-244 and :385-425)
 *   lr_mode: SAVFI_LR_SCALAR   lr[i] points at ONE float (LSLR: &table_i[num_step])
 *            SAVFI_LR_ELEMENT  lr[i] points at numel[i] floats (Meta-SGD)
 *   bc1[i], sqrt_bc2[i]: host float arrays with the per-tensor bias corrections
 *                   1-b1^step_i and sqrt(1-b2^step_i) (computed in double by the caller like
 *                   the reference does in Python floats, then rounded); ignored by SGD.
 *   beta1, beta2, eps are doubles so that (1-beta) is rounded to fp32 from the double
 *   difference, as the reference's Python-float arithmetic does.
 *   m, s: host arrays of device pointers (may be NULL for rules that do not use them).
 *   coef[i] (optional device float*, may be NULL array): when non-NULL the kernel also
 *   writes the per-element d out / d lr = -(update direction) so that the autograd
 *   backward w.r.t. lr is a plain product (see savfi_mt_update_bwd_f32).
 * ---------------------------------------------------------------------------------- */
#define SAVFI_RULE_SGD          0
#define SAVFI_RULE_ADAM         1
#define SAVFI_RULE_ADAMAX_LSLR  2
#define SAVFI_RULE_ADAMAX_MSGD  3
#define SAVFI_LR_SCALAR   0
#define SAVFI_LR_ELEMENT  1
#define SAVFI_MT_MAX_TENSORS 48

int savfi_mt_update_f32(int rule, int lr_mode, int n,
                        const float* const* w, const float* const* g, const float* const* lr,
                        float* const* m, float* const* s, float* const* out, float* const* coef,
                        const int64_t* numel, const float* bc1, const float* sqrt_bc2,
                        double beta1, double beta2, double eps, void* stream);

/* Backward of the update w.r.t. the learning rates (first-order MAML: g is a constant).
 *   dir[i] = the `coef` buffer written by the forward (= d out / d lr, per element), scale = 1;
 *            for SGD pass dir = g and scale = -1 (no coef buffer needed).
 *   lr_mode ELEMENT: g_lr[i][e]  = scale * g_out[i][e] * dir[i][e]
 *   lr_mode SCALAR : g_lr[i][0] += scale * sum_e g_out[i][e] * dir[i][e]   (one float per tensor,
 *                    accumulated with one atomic per workgroup: the caller zero-fills it)
 * g_w is the identity (g_w = g_out) and needs no kernel. */
int savfi_mt_update_bwd_f32(int lr_mode, int n,
                            const float* const* g_out, const float* const* dir, float* const* g_lr,
                            const int64_t* numel, float scale, void* stream);

/* L2F: per-tensor mean -> out_vec[i] (device float[n], zero-filled by the caller, accumulated
 * with one atomic per workgroup);  per-tensor scale out[i] = gamma[i]*w[i] (gamma: device
 * float[n]).  scale_bwd: g_w[i] = gamma[i]*g_out[i] (g_w may be NULL or hold NULL entries);
 * g_gamma[i] += sum_e g_out[i][e]*w[i][e] (zero-filled by the caller; may be NULL). */
int savfi_mt_mean_f32(int n, const float* const* x, const int64_t* numel, float* out_vec, void* stream);
int savfi_mt_scale_f32(int n, const float* const* w, const float* gamma, float* const* out,
                       const int64_t* numel, void* stream);
int savfi_mt_scale_bwd_f32(int n, const float* const* g_out, const float* const* w, const float* gamma,
                           float* const* g_w, float* g_gamma, const int64_t* numel, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused mean-reduced L1 / MSE loss and its gradient, `rows` independent reductions per launch:
 *   a, b [rows, n];  kind 0: result[r] = mean |a[r]-b[r]| ; kind 1: mean (a[r]-b[r])^2   (fully overwritten)
 *   `scratch`: savfi_l1_mse_scratch_floats(rows, n) floats of caller-owned device memory (per-workgroup partial sums,
 *   added in a fixed order: the value is bit-reproducible).
 *   bwd: g_a[r] = g_loss[r]*sign(a-b)/n or g_loss[r]*2*(a-b)/n.
 * rows = 1 is nn.L1Loss / nn.MSELoss (loss.py:287-290); rows > 1 serves the per-sample losses of tasks adapted in lockstep.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_l1_mse_scratch_floats(int rows, int64_t n);
int savfi_l1_mse_f32(int kind, const float* a, const float* b, float* result, float* scratch, int rows, int64_t n, void* stream);
int savfi_l1_mse_bwd_f32(int kind, const float* a, const float* b, const float* g_loss, float* g_a,
                         int rows, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused SSIM loss term and its gradient (csrc/ssim.hip), `rows` independent losses per launch:
 *   sr, hr [rows, C, H, W] (prediction, target); result[r] = (1 - mean SSIM map of row r) / 2, the map being the 11 x 11
 *   Gaussian-window (sigma 1.5), valid (unpadded) SSIM of pytorch_msssim: C (H - 10) (W - 10) values per row.
 *   H, W >= 11, SAVFI_E_SHAPE otherwise; rows * C <= 65535 and H * W < 2^31, SAVFI_E_TOOBIG otherwise.
 * The dynamic range L of C1 = (0.01 L)^2, C2 = (0.03 L)^2 is the reference's data-dependent rule, evaluated on the device
 * (no host read: capturable): range class = (min(sr) < -0.5 ? 1 : 0) | (max(sr) > 128 ? 2 : 0), L = 1, 2, 255, 256.
 *   range_mode SAVFI_SSIM_RANGE_PER_ROW   the rule on every row on its own (what `rows` calls on N = 1 tensors give)
 *              SAVFI_SSIM_RANGE_BATCH     the rule and the mean over all rows: ONE loss (what one call on an N = rows tensor gives);
 *                                         result, range_word and, in the backward, g_loss have one element, and the backward is
 *                                         called with rows = 1 and C = rows * C
 *              SAVFI_SSIM_RANGE_FIXED + k the class k = 0..3 whatever the data (k = 2: L = 255, the PSNR / SSIM metric)
 *   range_word[r]: the class the forward took (fully overwritten); the backward reads it, nothing else is kept.
 *   `scratch`: savfi_ssim_scratch_floats(rows, C, H, W) floats (per-workgroup partial sums added in a fixed order and partial
 *   extrema: the value is bit-reproducible; no atomics).
 *   bwd: g_sr [rows, C, H, W] = g_loss[r] * d result[r] / d sr (fully overwritten); the target gets no gradient.
 * ---------------------------------------------------------------------------------- */
#define SAVFI_SSIM_RANGE_PER_ROW 0
#define SAVFI_SSIM_RANGE_BATCH   1
#define SAVFI_SSIM_RANGE_FIXED   2
int64_t savfi_ssim_scratch_floats(int rows, int C, int H, int W);
int savfi_ssim_loss_f32(const float* sr, const float* hr, float* result, uint32_t* range_word, float* scratch, int rows, int C,
                        int H, int W, int range_mode, void* stream);
int savfi_ssim_loss_bwd_f32(const float* sr, const float* hr, const float* g_loss, const uint32_t* range_word, float* g_sr,
                            int rows, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * PSNR / SSIM evaluation metric (csrc/ssim.hip; utils.py:171-204 quantize + calc_psnr + ssim(val_range=255)), `rows` image pairs
 * per call, two launches (tile kernel, finish), no atomics, no cleared memory, no host read: capturable and bit-reproducible.
 *   pred, target [rows, C, H, W] in UNIT range.  Both are quantised as they are loaded, q = rint(clamp(x * 255, 0, 255)) (ties to
 *   even, what img.mul(255).clamp(0, 255).round() gives; +-inf clamp to 255 / 0); nothing quantised is written to memory.
 *   result[r][0] = mse  = (float)(S / (65025.0 C H W)) evaluated in double, S = sum (q_pred - q_target)^2, an exact integer
 *                         (PSNR = -10 log10(mse + 1e-8): the caller adds the reference's epsilon)
 *   result[r][1] = ssim = mean of the SSIM map with L = 255 (range class 2 of savfi_ssim_loss_f32: same window, same tap order,
 *                         partial sums added in a fixed order); exactly 1.0 for an identical pair.
 *   sq_sum[r] = S (may be NULL).  A NaN anywhere in a row makes both of that row's results NaN (and sq_sum[r] all ones).
 *   `scratch`: savfi_psnr_ssim_scratch_bytes(rows, C, H, W) bytes, 4-byte aligned, caller-owned.
 *   H, W >= 11, SAVFI_E_SHAPE otherwise; rows * C <= 65535 and H * W < 2^31, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_psnr_ssim_scratch_bytes(int rows, int C, int H, int W);
int savfi_psnr_ssim_f32(const float* pred, const float* target, float* result, unsigned long long* sq_sum, void* scratch,
                        int rows, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-scale SSIM and its gradient (csrc/ssim.hip; pytorch_msssim/__init__.py:78-104 "as implemented"), added under ABI 24.
 *   img1, img2 [rows, C, H, W] (prediction, target).  Five levels s = 0..4 on H >> s x W >> s images: the SSIM map and the map
 *   cs = v1 / v2 under the valid window of min(11, H_s, W_s) taps of gaussian(n, 1.5) centred at n / 2, then both images 2 x 2
 *   averaged (floor: an odd last row / column is dropped).  With the fp32 weights w = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333
 *     result[r] = mean(ssim_4) ^ (4 w_4) * prod_{s < 4} mean(cs_s) ^ w_s        (the reference's prod(pow1[:-1] * pow2[-1])),
 *   normalize != 0: every mean m replaced by (m + 1) / 2 first.  A negative base gives NaN, as the reference does.
 *   The reference pools once more after the fifth level and so raises below 32: H, W >= 32, SAVFI_E_SHAPE otherwise;
 *   rows * C <= 65535 and H * W < 2^31, SAVFI_E_TOOBIG otherwise.
 *   range_mode: the modes of savfi_ssim_loss_f32.  Without a fixed class the range rule is applied AGAIN ON EVERY LEVEL to that
 *   level's (pooled) prediction, per row (PER_ROW) or over everything (BATCH: one value, means over the whole batch, result and
 *   g_out have one element); FIXED + k holds on every level.
 *   quantize != 0: both images are quantised as savfi_psnr_ssim_f32 does while level 0 loads them (unit-range inputs; forward only;
 *   with FIXED + 2 this is msssim(quantize(pred), quantize(target), val_range=255)); nothing quantised is written.
 *   One launch per level (partial sums of both maps, the pooled pair of the next level and the partial extrema of its prediction)
 *   and a finish; plus the range pass of level 0 without a fixed class.  No atomics, no cleared memory, no host read: capturable
 *   and bit-reproducible.
 *   `scratch`: savfi_msssim_scratch_bytes(rows, C, H, W) bytes, 16-byte aligned, caller-owned, the same for every mode.  It starts
 *   with 16 32-bit words per result row (per row of the batch in PER_ROW / FIXED, one row in BATCH): float d result / d mean(ssim_s),
 *   s = 0..4 (zero for s < 4), float d result / d mean(cs_s) (zero for s = 4), uint32 range class of level s = 0..4, one spare.
 *   Then the pooled pairs, the gradients of the pooled predictions, partial sums and partial extrema.
 *   bwd: call with the forward's arguments and its scratch untouched.  g_img1 [rows, C, H, W] = g_out[r] * d result[r] / d img1,
 *   fully overwritten, coarse to fine with one launch per level: the level's own map gradient plus a quarter of the next-coarser
 *   level's, replicated (zero where the floor dropped a row / column).  img2 gets no gradient.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_msssim_scratch_bytes(int rows, int C, int H, int W);
int savfi_msssim_f32(const float* img1, const float* img2, float* result, void* scratch, int rows, int C, int H, int W,
                     int range_mode, int normalize, int quantize, void* stream);
int savfi_msssim_bwd_f32(const float* img1, const float* img2, const float* g_out, void* scratch, float* g_img1, int rows,
                         int C, int H, int W, int range_mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Laplacian-pyramid L1 loss term `Lap` and its gradient (csrc/laploss.hip), added under ABI 24.  `rows` independent losses per call.
 *   sr, hr [rows, C, H, W] (prediction, target); levels = L in 2..5 (SAVFI_E_UNSUPPORTED otherwise).
 *   g = [1, 4, 6, 4, 1] / 16, window g g^T per plane, borders by reflection about the border samples (pad 2).  c_0 = sr - hr and, for
 *   s = 0 .. L - 2 on H_s x W_s planes (H_0 = H, H_{s+1} = ceil(H_s / 2), W alike):
 *     c_{s+1} = (G c_s)[::2, ::2]        b_s = c_s - 4 G z_s,  z_s = zeros with c_{s+1} at the even positions, H_s x W_s
 *   and b_{L-1} = c_{L-1}.  result[r] = sum_s 2^s sum |b_s| / (C H W), sums over the planes of row r; fully overwritten.
 *   Every filtered level (s <= L - 2) needs H_s, W_s >= 3, SAVFI_E_SHAPE otherwise (L = 5: H, W >= 17; with `levels` out of range the
 *   shape is judged for the nearest legal value, so that SHAPE precedes UNSUPPORTED); rows * C <= 65535 and H * W < 2^31,
 *   SAVFI_E_TOOBIG otherwise.  One value over a batch: call with rows = 1 and C = N * C (the samples are further planes).
 *   One launch per filtered level and a finish.  Band elements are fp32; their sums are carried in double.  No atomics, no cleared
 *   memory, no host read: capturable and bit-reproducible.  Operands need 4-byte alignment only.
 *   `scratch`: savfi_laploss_scratch_bytes(rows, C, H, W, levels) bytes, 16-byte aligned, caller-owned.  In 32-bit words, every
 *   region rounded up to a multiple of four, P = rows * C:
 *     c_s, s = 1 .. L - 1:              P H_s W_s floats each
 *     g_{c_s}, s = 1 .. L - 2:          P H_s W_s floats each (written by the backward)
 *     partial sums, s = 0 .. L - 2:     one double (two words) per workgroup, P ceil(H_s / 32) ceil(W_s / 32) of them
 *   bwd: call with the forward's arguments and its scratch untouched.  g_sr [rows, C, H, W] = g_loss[r] * d result[r] / d sr, every
 *   element written once, coarse to fine with one launch per filtered level; sign(b_s) is recomputed from the c_s the forward left,
 *   by the forward's own device functions, and sign(0) = 0: an identical pair gives value 0 and gradient 0 exactly.  hr gets no gradient.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_laploss_scratch_bytes(int rows, int C, int H, int W, int levels);
int savfi_laploss_f32(const float* sr, const float* hr, float* result, void* scratch, int rows, int C, int H, int W, int levels,
                      void* stream);
int savfi_laploss_bwd_f32(const float* sr, const float* hr, const float* g_loss, void* scratch, float* g_sr, int rows, int C, int H,
                          int W, int levels, void* stream);

/* ------------------------------------------------------------------------------------
 * Census (soft ternary) loss term `Census` and its gradient (csrc/census.hip), added under ABI 24.  `rows` independent losses per
 * call, each the mean over `n` consecutive samples (n = 1: per sample; rows = 1, n = N: one value over a batch).
 *   sr, hr [rows * n, C, H, W] (prediction, target), C = 3 or 1, H, W >= 3.  Per sample:
 *     g = 0.2989 x_0 + 0.5870 x_1 + 0.1140 x_2 (C = 1: g = x_0), and g = 0 outside the frame (zero padding)
 *     for the 49 offsets o in {-3..3}^2:   d_o(p) = g(p + o) - g(p)        t_o(p) = d_o / sqrt(0.81 + d_o^2)
 *     delta_o = (t_o(sr) - t_o(hr))^2      h_o = delta_o / (0.1 + delta_o)   c(p) = sum_o h_o(p) / 49
 *     census = sum_p m(p) c(p) / (H W),    m(p) = 1 for 1 <= y <= H - 2 and 1 <= x <= W - 2, else 0
 *   result[r] = mean of census over the n samples of row r, fully overwritten.
 *   Errors, checked in this order before any launch: SAVFI_E_NULL; SAVFI_E_SHAPE (a dimension <= 0, H or W below 3);
 *   SAVFI_E_UNSUPPORTED (C not 1 or 3, an output pointer equal to an operand or to another output, a float pointer that is not 4-byte
 *   aligned or a scratch that is not 8-byte aligned); SAVFI_E_TOOBIG (rows * n > 65535 or H * W >= 2^31).
 *   Forward: one launch of 256-thread workgroups, one per tile of 8 rows x 32 columns per sample, one pixel per thread (the op is
 *   bound by its arithmetic, not by staging: small tiles spread a 256 x 448 frame over 448 workgroups), which stage the 14 x 38 gray
 *   patches of both images in LDS and leave one double each, and a finish launch.  Elements are fp32 (correctly rounded sqrt and
 *   division); sums are carried in double.
 *   `scratch`: savfi_census_scratch_bytes(rows, n, C, H, W) bytes, 16-byte aligned, caller-owned: one double per workgroup,
 *     partial[((r * n + i) * ceil(H / 8) + ty) * ceil(W / 32) + tx] = sum over tile (ty, tx) of sample i of row r of m(p) sum_o h_o(p),
 *   rows * n * ceil(H / 8) * ceil(W / 32) doubles, the total rounded up to a multiple of 16 bytes.  The finish adds a row's partials
 *   in that order (thread-strided, then one butterfly) and divides by 49 n H W once.
 *   bwd: ONE launch, nothing kept from the forward.  g_sr [rows * n, C, H, W] = g_loss[r] * d result[r] / d sr, every element written
 *   once, recomputed from the same patches by the forward's device functions; hr gets no gradient.
 *   No atomics, no cleared memory, no host read: capturable and bit-reproducible; an identical pair gives value 0 and gradient 0
 *   exactly.  All global accesses are scalar 4-byte ones: operands 4 or 8 bytes off a 16-byte boundary give the same bits.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_census_scratch_bytes(int rows, int n, int C, int H, int W);
int savfi_census_f32(const float* sr, const float* hr, float* result, void* scratch, int rows, int n, int C, int H, int W, void* stream);
int savfi_census_bwd_f32(const float* sr, const float* hr, const float* g_loss, float* g_sr, int rows, int n, int C, int H, int W,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * AdaCoF's deformable-tap op (adaptive collaboration of flows) and its parameter gradients (csrc/adacof.hip), added under ABI 24.
 *   x [N, C, Hp, Wp] the frame, padded by the caller: Hp = H + (F - 1) d, Wp = W + (F - 1) d, d = `dilation`; C = 3 or 1
 *   w, a, b [N, F^2, H, W]: per output pixel and tap t = k F + l (k, l in 0 .. F - 1) a weight, a vertical and a horizontal offset
 *   out [N, C, H, W], fully overwritten.  For pixel (y, x) and tap t:
 *     sy = float32(y + k d) + a_t            sx = float32(x + l d) + b_t        (ONE fp32 addition each: the coordinate IS fp32)
 *     sy <- min(max(sy, -1), Hp)             sx <- min(max(sx, -1), Wp)         (in float, before any conversion to an integer)
 *     iy = floor(sy), ty = sy - iy           ix = floor(sx), tx = sx - ix
 *     i0 = clamp(iy, 0, Hp - 1), i1 = clamp(iy + 1, 0, Hp - 1), j0, j1 likewise (border replicate)
 *     S_c = (1 - ty) ((1 - tx) x[c,i0,j0] + tx x[c,i0,j1]) + ty ((1 - tx) x[c,i1,j0] + tx x[c,i1,j1])
 *     out[n,c,y,x] = sum_t w_t S_c(t), the taps added in the order t = 0 .. F^2 - 1, product first
 *   bwd: ONE launch, nothing kept from the forward; g_out [N, C, H, W]; g_w, g_a, g_b [N, F^2, H, W], each fully overwritten, each
 *   may be NULL ("not wanted"), but not all three:
 *     g_w[t] = sum_c g_out[c] S_c(t)
 *     g_a[t] = w_t sum_c g_out[c] ((1 - tx) (x[i1,j0] - x[i0,j0]) + tx (x[i1,j1] - x[i0,j1]))
 *     g_b[t] = w_t sum_c g_out[c] ((1 - ty) (x[i0,j1] - x[i0,j0]) + ty (x[i1,j1] - x[i1,j0]))        (channels added in order)
 *   No gradient of x is built.  The float clamp changes no value (a coordinate beyond the border reads the border texel either way)
 *   and makes +-inf and +-1e30 offsets safe; where both indices of an axis clamp to one texel that offset's gradient is exactly 0.
 *   A NaN offset gives NaN in that pixel's out, in that tap's g_w and in both offset gradients of that tap, never a read outside x.
 *   Errors, checked in this order before any launch: SAVFI_E_NULL (an operand, or all three of g_w, g_a, g_b); SAVFI_E_SHAPE (one of
 *   N, C, H, W, F, dilation <= 0); SAVFI_E_UNSUPPORTED (C not 1 or 3, F even or above 11, dilation above 8, an output pointer equal
 *   to an operand or to another output, a pointer that is not 4-byte aligned); SAVFI_E_TOOBIG (N F^2 H W or N C Hp Wp >= 2^31).
 *   One launch each of 256-thread workgroups, one per tile of 4 rows x 64 columns per sample, one pixel per thread walking the F^2
 *   taps: the 3 F^2 parameter planes stream coalesced and non-temporally, the frame gathers go through the cache.  fp32, every
 *   operation rounded on its own (no contraction, no reassociation).  No atomics, no cleared memory, no host read: capturable and
 *   bit-reproducible.  All global accesses are scalar 4-byte ones: operands 4 bytes off a 16-byte boundary give the same bits.
 * ---------------------------------------------------------------------------------- */
int savfi_adacof_fwd_f32(const float* x, const float* w, const float* a, const float* b, float* out, int N, int C, int H, int W, int F,
                         int dilation, void* stream);
int savfi_adacof_bwd_f32(const float* x, const float* w, const float* a, const float* b, const float* g_out, float* g_w, float* g_a,
                         float* g_b, int N, int C, int H, int W, int F, int dilation, void* stream);

/* ------------------------------------------------------------------------------------
 * Softmax splatting: forward warping with a learned importance (Niklaus & Liu, CVPR 2020) and its gradients (csrc/softsplat.hip), added
 * under ABI 24.  This block is the specification; tests/softsplat_ref.py restates it in float64.
 *   x [N, C, H, W], flow [N, 2, H, W] (channel 0 horizontal, 1 vertical), metric Z [N, 1, H, W] (read in soft mode only; may be NULL
 *   otherwise), mode 0 = sum, 1 = avg, 2 = soft  ->  out [N, C, H, W], hit, den (D), mx (M) [N, 1, H, W], all four fully overwritten.
 *   Coordinates.  For the source pixel p = (i, j):  X = float32(j) + flow_x(p),  Y = float32(i) + flow_y(p)  (ONE fp32 addition each: the
 *   coordinate IS fp32).  x0 = floor(X), tx = X - x0, y0 = floor(Y), ty = Y - y0, all fp32.  The four corners q_k, k = 0 .. 3, are
 *   (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with the 1-D factors (1 - tx | tx) and (1 - ty | ty) and the bilinear weight
 *   b_k their product (factors and everything after them in double).  A corner TAKES PART only if it lies inside the frame and both of its
 *   1-D factors are > 0 (decided on the factors, not on their product).  All comparisons that keep a coordinate in range are made in float
 *   before any conversion to an integer.  A source whose flow is non-finite (in soft mode: or whose metric is), or whose target lies
 *   wholly outside, contributes nothing and receives zero gradients.
 *   Modes.  sum: out(q) = sum_p b_pq x(p).   avg: out = N / D with e = 1.
 *   soft: out_c(q) = N_c(q) / D(q),  N_c(q) = sum_p e_pq b_pq x_c(p),  D(q) = sum_p e_pq b_pq,  e_pq = expf(Z_p - M(q)),  M(q) = the
 *   maximum of Z_p over the sources taking part at q: a true per-target softmax, equal to sum exp(Z) b x / sum exp(Z) b but finite for
 *   every finite Z (the published implementations overflow above 88).  A `linear` mode is not built: soft with Z = log w expresses it.
 *   Where nothing lands out = 0, hit = 0, den = 0, mx = 0; elsewhere hit = 1.  den is sum e b in every mode (sum: sum b); mx is 0 outside
 *   soft mode.  hit carries no gradient.  If a sample of x holds a non-finite element, that whole sample of out is NaN (decided on the
 *   device; hit, den, mx do not depend on x).
 *   bwd: ONE launch, a gather per source pixel, no atomics; out, den, mx as the forward left them; g_out [N, C, H, W]; g_x [N, C, H, W],
 *   g_flow [N, 2, H, W], g_metric [N, 1, H, W], each fully overwritten, each may be NULL ("not wanted"), but not all three.
 *     s_k = sum_c g_c(q_k) (x_c(p) - out_c(q_k)) / D(q_k)            (sum mode: s_k = sum_c g_c(q_k) x_c(p), D = 1)
 *     g_x_c(p) = sum_k e_k b_k g_c(q_k) / D(q_k)       g_Z(p) = sum_k s_k e_k b_k       g_flow(p) = sum_k s_k e_k d b_k / d(X, Y)
 *   M is a constant (exact: out does not depend on it); a corner that did not take part contributes 0; g_metric is 0 outside soft mode.
 *   Errors, checked in this order before any launch: SAVFI_E_NULL (a required pointer; in bwd all three gradient outputs);
 *   SAVFI_E_SHAPE (one of N, C, H, W <= 0); SAVFI_E_UNSUPPORTED (C above 256, an unknown mode, soft mode without a metric, an output
 *   pointer equal to an operand or to another output, a float pointer that is not 4-byte aligned or a scratch that is not 8-byte
 *   aligned); SAVFI_E_TOOBIG (H W > 2^31 - 1 - 256, N > 65535 or N (C + 1) H W >= 2^40).  savfi_softsplat_scratch_bytes returns the same
 *   codes for its numbers.
 *   Forward, four launches: init (our own kernel, never a memset: a captured memset node clears only once), scan (per-sample maximum of
 *   |x| as an integer maximum of the bit patterns -> a power-of-two scale; the non-finite flag; in soft mode the scatter-max of Z onto the
 *   corners taking part, an integer maximum of an order-preserving key), scatter (one thread per source pixel and channel chunk;
 *   contributions formed in double, converted to 64-bit fixed point, rounded away from zero, added with 64-bit integer atomics: the
 *   denominator under the constant scale 2^(62 - ceil(log2(H W))) -- each share is at most 1 and at most H W reach a target -- the
 *   numerators under that scale divided by the power of two above the sample's largest |x|), finish.  No float atomics, no host read, no
 *   memset node: capturable and bit-reproducible, and each sample depends on itself alone.  expf, IEEE division, no contraction.
 *   `scratch`: savfi_softsplat_scratch_bytes(N, C, H, W) bytes, 8-byte aligned, caller-owned: int64 acc[N][C + 1][H W], uint32
 *   keys[N][H W], uint32 words[N][2], the total rounded up to a multiple of 16.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_softsplat_scratch_bytes(int N, int C, int H, int W);
int savfi_softsplat_fwd_f32(const float* x, const float* flow, const float* metric, float* out, float* hit, float* den, float* mx,
                            void* scratch, int N, int C, int H, int W, int mode, void* stream);
int savfi_softsplat_bwd_f32(const float* x, const float* flow, const float* metric, const float* out, const float* den, const float* mx,
                            const float* g_out, float* g_x, float* g_flow, float* g_metric, int N, int C, int H, int W, int mode,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Convolution epilogue: bias + activation, in place on the conv output z [N,C,H*W]:
 *   z <- act(z + bias[c]),  act(x) = x > 0 ? x : slope*x   (slope 0 ReLU, 0.2 LeakyReLU, 1 bias only)
 * bwd: gz = gy * act'(y) with y the forward OUTPUT (sign(y) == sign(z+b) for slope >= 0);
 *      gbias[c] = sum over n, hw of gz (may be NULL; fully overwritten; deterministic: per-workgroup partial sums
 *      go to `scratch` (caller-owned, savfi_bias_act_scratch_floats(N, C, HW) floats) and are added in a fixed order).
 *      gz may alias gy; gz may be NULL when only the bias gradient is wanted (slope 1: gz == gy).
 * ---------------------------------------------------------------------------------- */
int savfi_bias_act_fwd_f32(float* z, const float* bias, int N, int C, int HW, float slope, void* stream);
int64_t savfi_bias_act_scratch_floats(int N, int C, int HW);
int savfi_bias_act_bwd_f32(const float* gy, const float* y, float* gz, float* gbias, float* scratch,
                           int N, int C, int HW, float slope, void* stream);

/* ------------------------------------------------------------------------------------
 * Bilinear x2 up-sampling of `planes` = N*C maps [H,W] -> [2H,2W] with ATen's source-index rules
 * (align_corners 1: torch.nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True),
 *  sepconv/model.py:191,213-234;  0: F.interpolate(scale_factor=2, align_corners=False), voxel_flow.py:400-414).
 * bwd is the exact adjoint, computed as a gather (gin fully overwritten, deterministic).
 * ---------------------------------------------------------------------------------- */
int savfi_upsample2x_fwd_f32(const float* in, float* out, int planes, int H, int W, int align_corners, void* stream);
int savfi_upsample2x_bwd_f32(const float* gout, float* gin, int planes, int H, int W, int align_corners, void* stream);

/* Windowed form of the same map: `in` holds the crop rows [sy0,sy0+Hs) x cols [sx0,sx0+Ws) of the virtual
 * [planes,H,W] source, `out` the window rows [oy0,oy0+Hw) x cols [ox0,ox0+Ww) of the virtual [planes,2H,2W]
 * result (identical values to the full op on that window).  SAVFI_E_SHAPE if the window reads a source pixel
 * outside the crop.  bwd: gout is the window, gin the crop (fully overwritten; crop pixels no window output
 * reads get 0).  Used for SepConv's sub-networks (sepconv/model.py:196-245), whose 51-tap maps are consumed
 * only on the un-padded frame area (sepconv/model.py:346-349 crops the result). */
int savfi_upsample2x_window_fwd_f32(const float* in, float* out, int planes, int H, int W, int sy0, int sx0,
                                    int Hs, int Ws, int oy0, int ox0, int Hw, int Ww, int align_corners, void* stream);
int savfi_upsample2x_window_bwd_f32(const float* gout, float* gin, int planes, int H, int W, int sy0, int sx0,
                                    int Hs, int Ws, int oy0, int ox0, int Hw, int Ww, int align_corners, void* stream);
/* the same adjoint with the (leaky) ReLU derivative of the up-sampled map's PRODUCER folded into its store:
 *   gin[i] *= (y[i] > 0 ? 1 : slope),   y [planes,Hs,Ws] = that producer's activated output = the op's forward input (y == NULL: plain)
 * -- what autograd runs as ReLU's backward between the two (reference: nn.ReLU after the Subnets' third convolution and after every
 * Basic block in front of an Upsample, sepconv/model.py:172-245); here one element-wise pass over the map less. */
int savfi_upsample2x_window_bwd_masked_f32(const float* gout, const float* y, float slope, float* gin, int planes, int H, int W,
                                           int sy0, int sx0, int Hs, int Ws, int oy0, int ox0, int Hw, int Ww, int align_corners,
                                           void* stream);
/* Which kernel the adjoint entries above run for `planes` crops of Hs x Ws source pixels (the launcher asks the same function):
 *   0  one thread per source pixel (Ws < 32);   1  the LDS-tiled form;   8, 16, 32  the streaming form with strips of that many source
 *   rows -- the first of 32, 16, 8 at which cdiv(Ws, 64) * cdiv(Hs, rows) * planes >= 8192, the tiled form if none.
 * Host only: launches nothing, touches no device.  SAVFI_E_SHAPE for an argument <= 0.  tests/test_upsample_forms_gpu.py holds every
 * form to float64 and the forms to each other. */
int savfi_upsample2x_bwd_form(int planes, int Hs, int Ws);

/* ----------------------------------------------------------------------------------
 * 3x3 / stride 1 / zero-pad 1 convolution of the backbones (sepconv/model.py:172-245 Basic / Subnet /
 * Upsample blocks through model_utils.py:308-366 MetaConv2dLayer -> F.conv2d; cain, voxelflow likewise):
 * Winograd F(2x2,3x3) with its 16 batched GEMMs on the fp32 matrix cores, one fused kernel.
 *   mode 0  forward:        out[N,Co,H+2p-2,W+2p-2] = act(conv2d(x[N,Ci,H,W], w[Co,Ci,3,3], zero pad p) + bias)
 *                           (p = pad in {0,1}; bias may be NULL)
 *   mode 1  data gradient of that convolution:  x = gy[N,Co,H,W] -> out = gx[N,Ci,H+2-2p,W+2-2p]
 *                           (bias ignored, pass slope 1)
 * act(v) = v > 0 ? v : slope * v  (slope 1 = none, 0 = ReLU).  `workspace` is caller-owned device memory of
 * savfi_conv3x3_workspace_floats(same N, Ci, Co, H, W, pad, mode) floats; it receives the transformed filter and, for
 * deep layers whose reduction channels are split over workgroups, the partial outputs; it may be reused by the next
 * call on the same stream.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_conv3x3_workspace_floats(int N, int Ci, int Co, int H, int W, int pad, int mode);
int savfi_conv3x3_f32(const float* x, const float* w, const float* bias, float* out, float* workspace,
                      int N, int Ci, int Co, int H, int W, int pad, int mode, float slope, void* stream);

/* The same convolution for T tasks adapted in lockstep (the task loop of meta_learning_system.py:366 as ONE launch per
 * layer): T filter sets w [T,Co,Ci,3,3], bias [T,Co]; the N samples are ordered sample-major, sample n belongs to task
 * n % T and is convolved with that task's filters (N % T == 0).  T = 1 is savfi_conv3x3_f32. */
int64_t savfi_conv3x3_tasks_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad, int mode);
int savfi_conv3x3_tasks_f32(const float* x, const float* w, const float* bias, float* out, float* workspace,
                            int N, int T, int Ci, int Co, int H, int W, int pad, int mode, float slope, void* stream);

/* The two halves of savfi_conv3x3_tasks_f32, for a training step that runs the forward pass AND the data gradient on the
 * same filters (F.conv2d and its autograd backward, model_utils.py:308-366): the Winograd transform of both uses in ONE
 * launch, and the convolution on an already transformed filter.
 *   savfi_conv3x3_filters_f32      u_fwd / u_bwd (either may be NULL): the mode-0 / mode-1 transform of w [T,Co,Ci,3,3],
 *                                  savfi_conv3x3_filter_floats(T, Ci, Co, mode) floats each
 *   savfi_conv3x3_tasks_pre_f32    savfi_conv3x3_tasks_f32 with `u` (of the same mode) in place of w; `workspace`:
 *                                  savfi_conv3x3_tasks_pre_workspace_floats(...) floats (partial outputs of split
 *                                  launches; 0 for most shapes, then it may be NULL) */
int64_t savfi_conv3x3_filter_floats(int T, int Ci, int Co, int mode);
/* Layers of at most 512 -> 512 channels run on Winograd F(4x4, 3x3) (csrc/winograd4.h: 36 points per 4 x 4 outputs, a quarter of the
 * direct multiplies; fp32 rounding 3e-7 rms / <= 1e-5 max of the result's scale), deeper ones on F(2x2, 3x3).  The form follows the
 * channel counts alone, so a transformed filter is valid for every map size.  savfi_conv3x3_f4_workgroups: the workgroups the F(4x4)
 * kernel would launch for this call (32 tiles of 4 x 4 pixels x 32 produced channels each, x the reduction split of a deep layer on a
 * small map), 0 for an F(2x2) layer -- a caller with another kernel for launches that cannot fill the chip routes by this count. */
int64_t savfi_conv3x3_f4_workgroups(int N, int Ci, int Co, int H, int W, int pad, int mode);
/* The grid an F(4x4) launch of this call really has: each sample's row-major tile list is cut into groups of 32, so ceil(tiles / 32)
 * workgroups per sample, reduction split and 32-channel block -- fewer than the block count above on maps whose tile counts are no
 * powers of two (65 x 113 tiles: 230 against 255).  savfi_conv3x3_f4_workgroups keeps counting 2^(5-s) x 2^s tile BLOCKS: callers route
 * by it and routing does not move.  0 for an F(2x2) layer. */
int64_t savfi_conv3x3_f4_launched_workgroups(int N, int Ci, int Co, int H, int W, int pad, int mode);
/* Test hook: on != 0 makes the F(4x4) launches issued afterwards decode tiles by blocks again (the grid savfi_conv3x3_f4_workgroups
 * counts); 0 restores the flat tile lists.  Same results bit for bit either way.  *previous (may be NULL) receives the old setting. */
int savfi_conv3x3_debug_f4_block_decode(int on, int* previous);
/* The caller's choice of the form per layer AND map: bit 1 of every `mode` argument of the savfi_conv3x3_* functions (mode | 2) and `form`
 * = 2 below select the F(2x2) kernel whatever the channel counts -- for launches too small for F(4x4) to pay (it rounds 5x coarser; an
 * Adam-type inner rule turns that into flipped steps of elements whose gradient is rounding noise).  form = 0 / bit clear: by the channel
 * counts.  A transformed filter is valid for the form it was made for only.  The plain entry points are form 0. */
int savfi_conv3x3_filters_form_f32(const float* w, float* u_fwd, float* u_bwd, int T, int Ci, int Co, int form, void* stream);
int savfi_conv3x3_filters_multi_form_f32(const float* const* w, float* const* u_fwd, float* const* u_bwd, const int* T, const int* Ci,
                                         const int* Co, const int* form, int n, void* stream);
int savfi_conv3x3_dgrad_masked_form_f32(const float* gy, const float* u, const float* mask, float mask_slope, float* gx, float* workspace,
                                        int N, int T, int Ci, int Co, int H, int W, int pad, int form, void* stream);
int savfi_conv3x3_filters_f32(const float* w, float* u_fwd, float* u_bwd, int T, int Ci, int Co, void* stream);
/* n layers in one launch per 56 (layer, mode) jobs; entry i is savfi_conv3x3_filters_f32(w[i], u_fwd[i], u_bwd[i], T[i], Ci[i], Co[i]). */
int savfi_conv3x3_filters_multi_f32(const float* const* w, float* const* u_fwd, float* const* u_bwd, const int* T, const int* Ci,
                                    const int* Co, int n, void* stream);
int64_t savfi_conv3x3_tasks_pre_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad, int mode);
int savfi_conv3x3_tasks_pre_f32(const float* x, const float* u, const float* bias, float* out, float* workspace,
                                int N, int T, int Ci, int Co, int H, int W, int pad, int mode, float slope, void* stream);
/* savfi_conv3x3_tasks_pre_f32 for a layer whose activated result is average-pooled 2 x 2 right away (an encoder block's last layer).
 * pooled [N][channels of out][Ho / 2][Wo / 2] (floor sizes, as savfi_avgpool2x2_fwd_f32).  *did_pool = 1: the convolution's output
 * stage wrote it -- the values savfi_avgpool2x2_fwd_f32 computes from `out`, bit for bit, without reading `out` back; *did_pool = 0
 * (the F(2x2) form, a split reduction, an odd output width, a data gradient): `pooled` is untouched and the caller pools `out` itself. */
int savfi_conv3x3_tasks_pre_pool_f32(const float* x, const float* u, const float* bias, float* out, float* pooled, float* workspace,
                                     int N, int T, int Ci, int Co, int H, int W, int pad, int mode, float slope, int* did_pool,
                                     void* stream);
/* Data gradient (mode 1) on a transformed filter with the (leaky) ReLU derivative of the layer that PRODUCED this convolution's input
 * folded into the output stage: gx = dgrad(gy) * (mask > 0 ? 1 : mask_slope); mask [N,Ci,H+2-2pad,W+2-2pad] is the convolution's
 * forward input (= the producer's activated output).  conv -> ReLU -> conv chains (sepconv/model.py:172-245 Basic / Subnet blocks):
 * the producer's backward then needs no element-wise pass of its own.  workspace: as savfi_conv3x3_tasks_pre_f32, mode 1. */
int savfi_conv3x3_dgrad_masked_f32(const float* gy, const float* u, const float* mask, float mask_slope, float* gx,
                                   float* workspace, int N, int T, int Ci, int Co, int H, int W, int pad, void* stream);

/* savfi_conv3x3_tasks_pre_f32, forward (mode 0) only, with the result written UNIT-MAJOR: out[n] is [Ho][Wo / 16][Co][16] instead of
 * [Co][Ho][Wo] -- the 16-pixel units of the SepConv kernels with a unit's Co x 64 bytes contiguous (the layout `taps_unit16` of
 * savfi_sepconv_{fwd,bwd}_frames8_f32 reads).  The SepConv plugin's last Subnet convolution (reference sepconv/model.py:183-194: the
 * 51 -> 51 layer behind the bilinear x2) writes its taps this way.  Needs Wo % 16 == 0, a sample below 2^31 bytes and a launch without
 * a reduction split (savfi_conv3x3_unit16_supported says so: 1 / 0); SAVFI_E_UNSUPPORTED otherwise.  No workspace. */
int savfi_conv3x3_unit16_supported(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_tasks_pre_unit16_f32(const float* x, const float* u, const float* bias, float* out, int N, int T, int Ci, int Co,
                                       int H, int W, int pad, float slope, void* stream);
/* The data gradient of that layer on a cotangent that is unit-major as well: gy[n] is [H][W / 16][Co][16] (savfi_sepconv_bwd_frames8_f32 with
 * taps_unit16 = 3), gx [N][Ci][H+2-2pad][W+2-2pad] as always; u = the layer's data-gradient filter transform (savfi_conv3x3_filters_f32).
 * W % 16 == 0, no reduction split (savfi_conv3x3_in_unit16_supported: 1 / 0); SAVFI_E_UNSUPPORTED otherwise. */
int savfi_conv3x3_in_unit16_supported(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_dgrad_in_unit16_f32(const float* gy, const float* u, float* gx, int N, int T, int Ci, int Co, int H, int W, int pad,
                                      void* stream);

/* Weight gradient of the same convolution (zero padding `pad` in {0,1}), NCHW in and out, deterministic:
 *   gw[Co,Ci,3,3] = sum over n,y,x of gz[n,co,y,x] * x[n,ci,y+a-pad,x+b-pad]      x [N,Ci,H,W], gz [N,Co,H+2pad-2,W+2pad-2]
 * `workspace`: savfi_conv3x3_wgrad_workspace_floats(same N, Ci, Co, H, W, pad) floats of caller-owned device memory
 * (per-workgroup partial blocks, added in a fixed order). */
int64_t savfi_conv3x3_wgrad_workspace_floats(int N, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_wgrad_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int Ci, int Co,
                            int H, int W, int pad, void* stream);

/* Per-task weight gradients of T tasks in lockstep: gw [T,Co,Ci,3,3], gw[t] sums over the samples n with n % T == t. */
int64_t savfi_conv3x3_wgrad_tasks_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_wgrad_tasks_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int T, int Ci,
                                  int Co, int H, int W, int pad, void* stream);

/* The same weight gradient in Winograd form F(3x3, 2x2) (2.25x fewer multiplies; same contract, its own workspace size;
 * deterministic; sums in a different order than the direct form: results agree to fp32 rounding of the reduction). */
int64_t savfi_conv3x3_wgrad_wino_tasks_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_wgrad_wino_tasks_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int T, int Ci,
                                       int Co, int H, int W, int pad, void* stream);
/* ... and the bias gradient with it (round 5): gb [T][Co], gb[t][co] = sum of gz over the samples n % T == t and the map -- the gradient of
 * a bias added to this convolution's output (model_utils.py:308-366 MetaConv2dLayer: F.conv2d(..., bias)).  The weight gradient reads gz
 * anyway; the separate pass (savfi_bias_act_bwd_f32 with gz = NULL) read the whole map once more.  Sums in a fixed order (deterministic).
 * workspace: savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats(...) floats. */
int64_t savfi_conv3x3_wgrad_wino_tasks_bias_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_conv3x3_wgrad_wino_tasks_bias_f32(const float* x, const float* gz, float* gw, float* gb, float* workspace, int N, int T, int Ci,
                                            int Co, int H, int W, int pad, void* stream);

/* ----------------------------------------------------------------------------------
 * Direct K x K convolution, K in {3, 5, 7}, stride 1, zero padding `pad` (0 .. K-1), T filter sets (sample n uses set n % T):
 * F.conv2d of the backbones' layers that are not 3x3 (VoxelFlow's 5x5, Super SloMo's 7x7 / 5x5 heads) and of 3x3 layers where
 * Winograd rounding is not acceptable.  Arithmetic: every fp32 operand is split exactly into three bf16 pieces
 * (a = a1 + a2 + a3), the product sum runs as SIX bf16 MFMAs per K-slab (a1b1, a1b2, a2b1, a1b3, a3b1, a2b2) with fp32
 * accumulation: the dropped terms are < 2^-26 of a product, the result is as close to fp64 as an fp32 fmaf chain.
 *   savfi_convk_filters_f32     p_fwd / p_bwd (either may be NULL): w [T,Co,Ci,K,K] packed as bf16 triples in MFMA fragment
 *                               order for the forward pass (mode 0) / the data gradient (mode 1);
 *                               savfi_convk_filter_floats(T, Ci, Co, K, mode) 4-byte units each, caller-owned
 *   savfi_convk_tasks_pre_f32   mode 0: out[N,Co,H+2p-K+1,W+2p-K+1] = act(conv2d(x[N,Ci,H,W], w, pad p) + bias[T,Co])
 *                               mode 1: x = gy[N,Co,H,W] -> out = gx[N,Ci,H+K-1-2p,W+K-1-2p]   (bias ignored, pass slope 1)
 *                               `packed` = the buffer of the same mode from savfi_convk_filters_f32
 *                               `precise` != 0: the five cross terms accumulate apart from the a1b1 sum (3x closer to float64
 *                               than an fp32 fmaf chain; for networks that amplify convolution rounding, ~10-15 % slower)
 * ---------------------------------------------------------------------------------- */
int64_t savfi_convk_filter_floats(int T, int Ci, int Co, int K, int mode);
int savfi_convk_filters_f32(const float* w, float* p_fwd, float* p_bwd, int T, int Ci, int Co, int K, void* stream);
/* The same for n layers in ONE launch per 56 (layer, mode) jobs: arrays of n pointers / shapes (host memory); entry i is
 * savfi_convk_filters_f32(w[i], p_fwd[i], p_bwd[i], T[i], Ci[i], Co[i], K[i]).  A MAML inner step re-packs every layer's fast weights
 * after every update (reference: nothing to pack -- F.conv2d reads the fast weight, model_utils.py:354-366); one launch per step
 * instead of one per layer and pass. */
int savfi_convk_filters_multi_f32(const float* const* w, float* const* p_fwd, float* const* p_bwd, const int* T, const int* Ci,
                                  const int* Co, const int* K, int n, void* stream);
int savfi_convk_tasks_pre_f32(const float* x, const float* packed, const float* bias, float* out, int N, int T, int Ci,
                              int Co, int H, int W, int K, int pad, int mode, float slope, int precise, void* stream);
/* the same fold for the direct kernels: gx = savfi_convk_tasks_pre_f32(mode 1)(gy) * (mask > 0 ? 1 : mask_slope).  K = 3 and
 * precise = 0 only (the layers of the conv -> act -> conv chains); SAVFI_E_UNSUPPORTED otherwise: the caller masks the plain data
 * gradient itself (savfi_bias_act_bwd_f32 without bias), as hip_ops.convk_tasks_pre does. */
int savfi_convk_dgrad_masked_f32(const float* gy, const float* packed, const float* mask, float mask_slope, float* gx, int N, int T,
                                 int Ci, int Co, int H, int W, int K, int pad, int precise, void* stream);
/* `reflect` != 0 (mode 0 only, pad < H, W): the border of width `pad` mirrors the image instead of reading zeros, i.e.
 * conv2d(nn.ReflectionPad2d(pad)(x), w) without the padded copy -- CAIN's MetaConvNorm (reference model_utils.py:821-848).  Its data
 * gradient is savfi_convk_tasks_pre_f32(mode 1, pad 0) on gy (the gradient of the padded extent) folded by
 * savfi_reflect_pad_bwd_f32; its weight gradient savfi_convk_wgrad_tasks_reflect_f32. */
int savfi_convk_tasks_pre_reflect_f32(const float* x, const float* packed, const float* bias, float* out, int N, int T, int Ci,
                                      int Co, int H, int W, int K, int pad, int mode, float slope, int precise, int reflect,
                                      void* stream);
/* gx[planes,H,W] = adjoint of nn.ReflectionPad2d(pad) applied to gp[planes,H+2pad,W+2pad] (gather: deterministic, no zero fill) */
int savfi_reflect_pad_bwd_f32(const float* gp, float* gx, int planes, int H, int W, int pad, void* stream);
/* the same fold plus a second cotangent of the unpadded map: gx = fold(gp) + add (add[planes,H,W]; NULL = savfi_reflect_pad_bwd_f32).
 * CAIN's RCAB (reference model_utils.py:957-990) pads x for its first convolution and adds x to its result: both gradients of x in
 * one pass (ABI 20) */
int savfi_reflect_pad_bwd_add_f32(const float* gp, const float* add, float* gx, int planes, int H, int W, int pad, void* stream);
/* xp[planes,H+2pad,W+2pad] = nn.ReflectionPad2d(pad)(x[planes,H,W]) (reference model_utils.py:829, :838), pad < H, W: the padded copy
 * the Winograd kernels read (ABI 20) */
int savfi_reflect_pad_fwd_f32(const float* x, float* xp, int planes, int H, int W, int pad, void* stream);

/* Weight gradient of the same convolution (same arithmetic; deterministic: per-workgroup partial blocks added in a fixed order):
 *   gw[T,Co,Ci,K,K], gw[t] = sum over samples n with n % T == t, y, x of gz[n,co,y,x] * x[n,ci,y+ky-pad,x+kx-pad]
 *   x [N,Ci,H,W], gz [N,Co,H+2pad-K+1,W+2pad-K+1]; `workspace`: savfi_convk_wgrad_workspace_floats(...) floats, caller-owned. */
int64_t savfi_convk_wgrad_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int K, int pad);
int savfi_convk_wgrad_tasks_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int T, int Ci, int Co,
                                int H, int W, int K, int pad, int precise, void* stream);
/* the same with x's border of width `pad` mirrored (see savfi_convk_tasks_pre_reflect_f32) */
int savfi_convk_wgrad_tasks_reflect_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int T, int Ci, int Co,
                                        int H, int W, int K, int pad, int precise, int reflect, void* stream);
/* the same (precise = 0) that also hands out the bias gradient gb [T,Co] = sums of gz over the samples n % T == t and the map: the sums ride
 * on the kernel's staging of gz (fixed order, bit-reproducible; gw is bit-identical to the call above), which saves the bias pass over
 * the map (reference: the bias gradient autograd returns for MetaConv2dLayer's F.conv2d, model_utils.py:308-366).  Only for the shapes
 * savfi_convk_wgrad_sums_bias() answers 1 for (3 x 3 layers of >= 48 -> 48 channels: the all-taps kernel, csrc/convk_wgrad.hip);
 * SAVFI_E_UNSUPPORTED otherwise.  Same workspace as above. */
int savfi_convk_wgrad_sums_bias(int N, int T, int Ci, int Co, int H, int W, int K, int pad);
int savfi_convk_wgrad_tasks_bias_f32(const float* x, const float* gz, float* gw, float* gb, float* workspace, int N, int T, int Ci, int Co,
                                     int H, int W, int K, int pad, int reflect, void* stream);

/* The 3 x 3 weight gradient (same contract and arithmetic as savfi_convk_wgrad_tasks_f32, K = 3, pad 0 or 1) for maps of at most 32
 * output columns (SAVFI_E_UNSUPPORTED beyond): a workgroup keeps a band of rows of both operands in LDS and issues all nine taps of the
 * band between two barriers (csrc/convk_wgrad.hip, convk_wgrad3_small); added under ABI 24.  With at least one 64 x 64 channel block per
 * CU the kernel writes gw (and gb) itself: one launch, the workspace query answers 0 and `workspace` may be NULL; otherwise the
 * (sample, band) list is cut into parts whose blocks savfi_convk_wgrad's reduction adds in a fixed order.  Bit-reproducible.
 *   savfi_convk_wgrad3_small_plan: the plan, on the host (cus > 0: for that many CUs, needs no device; cus <= 0: the device's).
 *     out[0] rows of a band, out[1] bands of a map (band b = rows b out[0] .. min(Ho, (b + 1) out[0]) - 1), out[2] bytes of LDS of a
 *     workgroup, out[3] parts of the (sample, band) list, out[4] 1 = gw and gb written by the kernel itself (exactly when
 *     out[5] >= cus), out[5] channel blocks T ceil(Co / 64) ceil(Ci / 64), out[6] (sample, band) items of a filter set,
 *     out[7] 32-pixel K-steps of a band.
 *   savfi_convk_wgrad3_small_route: 1 where savfi_conv3x3_wgrad_wino_tasks_f32 / _bias_f32 hand their call to this kernel
 *     (Ci, Co >= 256, at most 32 output columns and 768 output pixels; 0 everywhere in a -DSAVFI_WGRAD_SMALL=0 build). */
int savfi_convk_wgrad3_small_plan(int N, int T, int Ci, int Co, int H, int W, int pad, int cus, int* out /* [8] */);
int savfi_convk_wgrad3_small_route(int N, int T, int Ci, int Co, int H, int W, int pad);
int64_t savfi_convk_wgrad3_small_workspace_floats(int N, int T, int Ci, int Co, int H, int W, int pad);
int savfi_convk_wgrad3_small_tasks_f32(const float* x, const float* gz, float* gw, float* workspace, int N, int T, int Ci, int Co,
                                       int H, int W, int pad, void* stream);
int savfi_convk_wgrad3_small_tasks_bias_f32(const float* x, const float* gz, float* gw, float* gb, float* workspace, int N, int T,
                                            int Ci, int Co, int H, int W, int pad, void* stream);

/* ----------------------------------------------------------------------------------
 * Channel attention + residual of CAIN's RCAB (model_utils.py:931-953 MetaCALayer, :957-990 MetaRCAB):
 *   s = mean_hw(t);  y = sigmoid(W2 relu(W1 s + b1) + b2);  out = t * y + x        t, x, out [N,C,H,W]; T weight sets (n % T)
 *   savfi_ca_pool_f32       s[plane] = scale * sum_hw a[plane][.] (* b[plane][.] when b != NULL)       planes = N*C
 *   savfi_ca_mlp_fwd_f32    y [N,C], a1 [N,Cr] (hidden activations, kept for the backward) from s [N,C]; w1 [T,Cr,C], b1 [T,Cr],
 *                           w2 [T,C,Cr], b2 [T,C]; C <= 1024, Cr <= 64
 *   savfi_ca_mlp_bwd_f32    r [N,C] = sum_hw g*t  ->  ds [N,C] (gradient w.r.t. s, times inv_hw) and gw1, gb1, gw2, gb2 per task
 *   savfi_ca_apply_f32      out = a * y[plane] + x          (x != NULL: forward, x = the skip connection)
 *                           out = a * y[plane] + ds[plane]  (x == NULL: backward, gradient w.r.t. t)
 * ---------------------------------------------------------------------------------- */
int savfi_ca_pool_f32(const float* a, const float* b, float* s, int64_t planes, int hw, float scale, void* stream);
int savfi_ca_mlp_fwd_f32(const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* a1,
                         int N, int T, int C, int Cr, void* stream);
int savfi_ca_mlp_bwd_f32(const float* r, const float* s, const float* y, const float* a1, const float* w1, const float* w2,
                         float* ds, float* gw1, float* gb1, float* gw2, float* gb2, int N, int T, int C, int Cr, float inv_hw,
                         void* stream);
int savfi_ca_apply_f32(const float* a, const float* y, const float* x, const float* ds, float* out, int64_t planes, int hw,
                       void* stream);
/* forward of the same block with the MLP inside the apply launch (Cr <= 16, C <= 256; SAVFI_E_UNSUPPORTED otherwise: the two calls
 * above): out = a * y + x with y = sigmoid(W2 relu(W1 s + b1) + b2) of the sample, s [N,C] from savfi_ca_pool_f32; y [N,C] and
 * a1 [N,Cr] are written for the backward, bit-identical to savfi_ca_mlp_fwd_f32's (ABI 20) */
int savfi_ca_apply_mlp_f32(const float* a, const float* s, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* x, float* out, float* y, float* a1, int N, int T, int C, int Cr, int hw, void* stream);
/* backward of the same with the MLP's backward inside the apply launch (same limits): gt = g * y + ds, ds recomputed per workgroup,
 * r [N,C] = sum_hw g * t from savfi_ca_pool_f32; gw1 [T,Cr,C], gb1 [T,Cr], gw2 [T,C,Cr], gb2 [T,C] from T workgroups at the front of
 * the grid; the parameter gradients bit-identical to savfi_ca_mlp_bwd_f32's, gt within an ulp of savfi_ca_mlp_bwd_f32 +
 * savfi_ca_apply_f32 (ABI 20) */
int savfi_ca_apply_bwd_mlp_f32(const float* g, const float* r, const float* s, const float* y, const float* a1, const float* w1,
                               const float* w2, float* gt, float* gw1, float* gb1, float* gw2, float* gb2, int N, int T, int C, int Cr,
                               int hw, void* stream);

/* ----------------------------------------------------------------------------------
 * Per-plane mean removal of CAIN's input frames (model_utils.py:11-15 sub_mean; cain/model.py:70-94):
 *   mean[p] = sum_i x[p][i] / hw;  out[p][i] = x[p][i] - mean[p]            x, out [planes][hw] (out may alias x), mean [planes]
 * Two launches, fixed summation order, no cleared memory (safe inside a captured hipGraph, where ATen's multi-workgroup
 * reduction is not: csrc/submean.hip).  `workspace`: savfi_sub_mean_workspace_floats(planes, hw) floats, caller-owned.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_sub_mean_workspace_floats(int64_t planes, int hw);
int savfi_sub_mean_f32(const float* x, float* out, float* mean, float* workspace, int64_t planes, int hw, void* stream);

/* ----------------------------------------------------------------------------------
 * Frame staging (data/vimeo_septuplet.py:68-80, data/video.py:44-51: channel swap, HWC->CHW, .float()/255,
 * Normalize): src = N decoded frames, uint8 [N,H,W,3] on the DEVICE (copied there as bytes);
 * dst[n][c][y][x] = (src[n][y][x][swap_rb ? 2-c : c] / div - mean_c) / std, fp32 [N,3,H,W]; one mean per OUTPUT
 * channel (Super SloMo subtracts 0.429 / 0.431 / 0.397, data/vimeo_septuplet.py:31-35).
 * ---------------------------------------------------------------------------------- */
int savfi_frames_u8_to_f32(const unsigned char* src, float* dst, int64_t N, int H, int W, int swap_rb, float div,
                           float mean_c0, float mean_c1, float mean_c2, float std, void* stream);

/* ----------------------------------------------------------------------------------
 * Frame writer (utils.py:276-285 save_image, :171-172 quantize): src fp32 [N,C,H,W] in unit range ->
 * dst[n][y][x][c] = rint(clamp(src[n][c][y][x] * 255, 0, 255)) as uint8 [N,H,W,C] on the DEVICE, so that a frame leaves it as
 * bytes.  The same quantisation as savfi_psnr_ssim_f32 (one device function); a NaN is written as 0.  C = 1 or 3,
 * SAVFI_E_UNSUPPORTED otherwise.
 * ---------------------------------------------------------------------------------- */
int savfi_frames_f32_to_u8(const float* src, unsigned char* dst, int64_t N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * DAIN's adaptive warping layer (csrc/dainwarp.hip; FilterInterpolation/filterinterpolation_cuda_kernel.cu:29-460), ABI 24.
 *   in [B,C,H,W], flow [B,2,H,W], filt [B,16,H,W], out / gout / g_in [B,C,H,W], g_flow [B,2,H,W], g_filt [B,16,H,W].
 *   Per pixel (w_i, h_i), all in fp32: x2 = w_i + fx, y2 = h_i + fy; valid iff x2 >= 0 && y2 >= 0 && x2 <= W-1 && y2 <= H-1 &&
 *   |fx| < W/2.f && |fy| < H/2.f (a NaN flow is invalid).  Valid: the 4 x 4 window with origin (int(x2)-1, int(y2)-1), rows and
 *   columns clamped into the image for `in` only, tap (j,i) weighted with filt channel 4j+i; rows 0-1 "top", columns 0-1 "left";
 *   out = (1-a)(1-b) TL + a(1-b) TR + (1-a)b BL + ab BR, a = x2 - int(x2), b = y2 - int(y2).  Invalid: out = in at that pixel.
 *   Backward: g_in and g_filt are the adjoints of the valid branch; g_flow_x = sum_c g ((1-b)(TR-TL) + b(BR-BL)),
 *   g_flow_y = sum_c g ((1-a)(BL-TL) + a(BR-TR)); an invalid pixel gives NO gradient to anything, `in` included (kept from
 *   the reference).  g_in, g_flow, g_filt may each be NULL (skipped); every gradient that is written is written completely, and
 *   the entry zeroes g_in itself (with a kernel).  Forward, g_flow and g_filt are bit-reproducible; g_in is accumulated with fp32
 *   atomicAdd in arrival order, as in the reference, and is not.
 *   filter_size != 4: SAVFI_E_UNSUPPORTED.  H*W <= 2^31 - 257, B, C <= 65535 and B*C*H*W < 2^40, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int savfi_filterinterp_fwd_f32(const float* in, const float* flow, const float* filt, float* out, int B, int C, int H, int W,
                               int filter_size, void* stream);
int savfi_filterinterp_bwd_f32(const float* in, const float* flow, const float* filt, const float* gout, float* g_in /*nullable*/,
                               float* g_flow /*nullable*/, float* g_filt /*nullable*/, int B, int C, int H, int W, int filter_size,
                               void* stream);
/* The forward into a channel slice, added under ABI 24: out is [B,C_total,H,W] and the call writes out[b][c_off + c][y][x], c < C, with
 * the arithmetic of savfi_filterinterp_fwd_f32 in its order (the same bits, the pass-through of an invalid pixel included); every
 * other channel of `out` is left as it was.  One launch, no memset, no atomics: capturable.  c_off < 0 or c_off + C > C_total:
 * SAVFI_E_SHAPE; the limits above hold for C and for C_total (B*C_total*H*W < 2^40, the OUTPUT's elements). */
int savfi_filterinterp_fwd_slice_f32(const float* in, const float* flow, const float* filt, float* out, int B, int C, int H, int W,
                                     int filter_size, int C_total, int c_off, void* stream);

/* ------------------------------------------------------------------------------------
 * DAIN's depth-aware flow projection (csrc/dainwarp.hip; DepthFlowProjection/depthflowprojection_cuda_kernel.cu:29-341), ABI 24.
 *   flow [B,2,H,W], w [B,1,H,W] (the depth inverse), count [B,1,H,W] and out [B,2,H,W] (both written completely).
 *   Scatter: a source with x2, y2 inside [0,W-1] x [0,H-1] adds -w fx, -w fy and w to the targets (T,L), (T,R), (Bt,L), (Bt,R),
 *   L = int(x2), T = int(y2), R = min(L+1, W-1), Bt = min(T+1, H-1) -- a doubled target is hit twice.  Average: out /= count where
 *   count > 0.  fillhole != 0: a pixel with count <= 0 becomes the unweighted mean of out at the first pixel with non-zero count
 *   to its left, right, top and bottom, over those of them with count > 0; 0 when there is none.
 *   The sums are accumulated as 64-bit fixed-point integers (per-sample power-of-two scale from a device-side maximum, every
 *   contribution rounded away from zero), so count, out and every decision taken from them are bit-reproducible.
 *   `scratch`: savfi_depthflowproj_scratch_bytes(B, H, W) bytes, 8-byte aligned (SAVFI_E_UNSUPPORTED otherwise), caller-owned,
 *   cleared by a kernel of the entry.  Five launches (four without the fill), no host read: capturable.
 *   A source whose |w| max(|fx|, |fy|, 1) is not finite in fp32 (a NaN / Inf depth inverse, or |w| beyond ~1e29 times the flow) has
 *   no fixed-point value: it is not scattered and does not set the scale.
 *   Backward (a gather over the same targets; g_flow and g_w may each be NULL (skipped), one that is written is written completely;
 *   zero at sources the validity test left out):
 *   g_flow = -sum_t g_t w / count_t;  g_w = -sum_t sum_{x,y} g_t / count_t (f - out_t), as the reference writes it.
 *   H*W <= 2^31 - 257, B <= 65535 and 3*B*H*W < 2^40, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_depthflowproj_scratch_bytes(int B, int H, int W);
int savfi_depthflowproj_fwd_f32(const float* flow, const float* w, float* count, float* out, void* scratch, int B, int H, int W,
                                int fillhole, void* stream);
int savfi_depthflowproj_bwd_f32(const float* flow, const float* w, const float* count, const float* out, const float* gout,
                                float* g_flow /*nullable*/, float* g_w /*nullable*/, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * PWC-Net's correlation (csrc/correlation.hip; correlation_package_pytorch1_0/correlation_cuda_kernel.cu), added under ABI 24.
 *   f1, f2, g1, g2 [N,C,H,W]; out, gout [N,(2md+1)^2,H,W].  The reference's pad_size = max_displacement = md, kernel_size = 1,
 *   stride1 = stride2 = 1, corr_multiply = 1; md = 4 only (SAVFI_E_UNSUPPORTED otherwise).  p = the input with md zeros around it:
 *     out[n,tc,y,x] = (1/C) sum_c p1[n,c,y,x] p2[n,c,y+tj,x+ti],  tj, ti in -md..md,  tc = (tj+md)(2md+1) + (ti+md),
 *   channels summed in order in fp32, divided by C, then out = out > 0 ? out : slope * out (slope = 1: no activation).  A
 *   displacement that leaves the frame is multiplied by the padded zero, not skipped: a NaN / inf of f1 gives NaN in all 81 channels.
 *   NCHW is read in place (no padded channels-last copies).  Every output element is written; no memset, no atomics.
 *   Backward: ge = gout * (out > 0 ? 1 : slope) when `out` (the forward's result, run with the same slope) is given, gout otherwise;
 *     g1[n,c,y,x] = (1/C) sum_tc ge[n,tc,y,x] p2[n,c,y+tj,x+ti]             (never skipped: padded zeros)
 *     g2[n,c,y,x] = (1/C) sum_tc ge[n,tc,y-tj,x-ti] f1[n,c,y-tj,x-ti]       (over the tc whose source pixel is inside the frame)
 *   both as gathers with sequential fp32 sums over tc.  g1 or g2 may be NULL (skipped; with both NULL nothing is launched).
 *   Forward and backward are bit-reproducible and capturable.
 *   H*W <= 2^31 - 257, H <= 4 * 65535, N, C <= 65535, N * ceil(C/16) <= 65535 and N * max(C, 81) * H*W < 2^40, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int savfi_correlation_fwd_f32(const float* f1, const float* f2, float* out, int N, int C, int H, int W, int md, float slope,
                              void* stream);
int savfi_correlation_bwd_f32(const float* f1, const float* f2, const float* gout, const float* out /*nullable*/, float slope,
                              float* g1 /*nullable*/, float* g2 /*nullable*/, int N, int C, int H, int W, int md, void* stream);

/* ------------------------------------------------------------------------------------
 * PWC-Net's warp (csrc/correlation.hip; dain/PWCNet/PWCNet.py:158-198), added under ABI 24.  Forward only.
 *   img, out [N,C,H,W], flow [N,2,H,W] in pixels, `scale` the level's flow scale (the reference's `up_flow * 0.625` etc.).
 *   out = bilinear(img, ix, iy) * (mask >= 0.9999f ? 1 : 0), mask = the same bilinear sample of an all-ones image, with, each step one
 *   fp32 operation:  vx = x + flow_x * scale;  nx = 2 vx / max(W-1, 1) - 1;  ix = ((nx + 1) / 2) (W - 1)   (grid_sample with
 *   align_corners=True, as the torch the reference pins runs it), likewise in y;  x0 = floor(ix);  weights nw = (x0+1-ix)(y0+1-iy),
 *   ne = (ix-x0)(y0+1-iy), sw = (x0+1-ix)(iy-y0), se = (ix-x0)(iy-y0);  image and mask sums in the order nw, ne, sw, se over the
 *   corners inside the frame (one outside is skipped).  A NaN / inf position samples nothing: mask = 0, out = 0.
 *   H*W <= 2^31 - 257, N, C <= 65535, N * ceil(C/8) <= 65535 and N*C*H*W < 2^40, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int savfi_pwcwarp_fwd_f32(const float* img, const float* flow, float scale, float* out, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------
 * DAIN's frozen front and rectify net (csrc/dainnet.hip, csrc/loss.hip), added under ABI 24.  Forward only unless said otherwise;
 * float32 NCHW read in place; no memset, no atomics; bit-reproducible and capturable.  Every entry validates before it launches:
 * NULL, then SHAPE, then UNSUPPORTED, then TOOBIG.
 *
 * Train-mode BatchNorm2d + ReLU.  x [N,C,H,W]; a GROUP is n_per_group consecutive samples (N % n_per_group == 0) and has statistics
 * of its own: mean[g * stat_stride + c], var[g * stat_stride + c] (biased variance) over its n_per_group * H * W values, which must
 * be at least 2 (SAVFI_E_SHAPE for a count of 1, as torch raises).  Two passes (mean, then centred squares) in a summation order that
 * depends on (n_per_group, H, W) alone: a group's statistics are the same bits whatever else the batch holds and wherever the tensor
 * lies.  scratch: savfi_bn_stats_scratch_floats floats (0: none needed, scratch may be NULL).
 *   savfi_bn_apply_relu_f32: out[n, c_off + c] = relu((x[n,c] - mean) / sqrt(var + eps) * gamma[c] + beta[c]) into an output of
 *   C_total >= c_off + C channels (the other channels are not touched); gamma / beta may be NULL (1 / 0); statistics of group
 *   n / n_per_group.  Eval mode: the running buffers with n_per_group = N and stat_stride = 0.
 *   savfi_bn_running_update_f32: running[i][:] = (1 - momentum) running[i][:] + momentum * (stat[i][:] * unbias[i]) for n buffers of
 *   numel[i] floats (host arrays of device pointers / sizes / factors; unbias NULL = 1), ceil(n / SAVFI_MT_MAX_TENSORS) launches.
 * N, C <= 65535, H*W <= 2^31 - 1025, N * C_total * H*W < 2^40, SAVFI_E_TOOBIG otherwise.
 * ---------------------------------------------------------------------------------- */
int64_t savfi_bn_stats_scratch_floats(int N, int C, int H, int W, int n_per_group);
int savfi_bn_stats_f32(const float* x, float* mean, float* var, int64_t stat_stride, float* scratch /*nullable*/, int N, int C, int H, int W,
                       int n_per_group, void* stream);
int savfi_bn_apply_relu_f32(const float* x, const float* mean, const float* var, int64_t stat_stride, const float* gamma /*nullable*/,
                            const float* beta /*nullable*/, float eps, float* out, int N, int C, int H, int W, int n_per_group, int c_off,
                            int C_total, void* stream);
int savfi_bn_running_update_f32(int n, float* const* running, const float* const* stat, const int64_t* numel, const float* unbias,
                                float momentum, void* stream);

/* nn.MaxPool2d(2, 2) of `planes` planes [H,W] -> [H/2, W/2] (odd sides floor; H, W >= 2); ATen's scan (rows, then columns, a NaN
 * replaces the running maximum), so NaN propagates with ATen's bits.  planes <= 65535. */
int savfi_maxpool2x2_f32(const float* in, float* out, int64_t planes, int H, int W, void* stream);

/* out = skip + UpsamplingNearest2d(2)(low): low [planes,h,w], skip / out [planes,H,W] with H == 2h and W == 2w exactly
 * (SAVFI_E_SHAPE otherwise).  planes <= 65535. */
int savfi_upnearest2x_add_f32(const float* low, const float* skip, float* out, int64_t planes, int h, int w, int H, int W, void* stream);

/* y = relu(a + r) over n floats (NaN kept).  Its derivative is savfi_bias_act_bwd_f32 on y, for both inputs. */
int savfi_add_relu_f32(const float* a, const float* r, float* y, int64_t n, void* stream);

/* Charbonnier loss: result[row] = mean_i sqrt((a - b)^2 + eps^2) for `rows` rows of n floats, on the row reduction of
 * savfi_l1_mse_f32 (scratch: savfi_l1_mse_scratch_floats(rows, n)); eps > 0.  Backward: g_a = g_loss[row] / n * d / sqrt(d^2 + eps^2),
 * exactly 0 where d == 0 (g_b = -g_a). */
int savfi_charbonnier_f32(const float* a, const float* b, float* result, float* scratch, int rows, int64_t n, float eps, void* stream);
int savfi_charbonnier_bwd_f32(const float* a, const float* b, const float* g_loss, float* g_a, int rows, int64_t n, float eps,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAVFI_HIP_H_ */
