/* libvp_hip.so - C ABI of the MI355X-native voicepuppet hot path.
 *
 * The reference (taylorlu/voicepuppet) has no FFI boundary for its neural path: it is TF1.x graph
 * construction behind Python classes.  Its one native precedent is utils/cython/mesh_core.h:53-77
 * (free functions, raw pointers + explicit int sizes, caller owns every buffer).  This header keeps
 * that convention for the path BASELINE.json names:
 *
 *   vp_pixrefer_*   replaces  voicepuppet/pixrefer/pixrefer.py:59-438   (PixReferNet.build_network,
 *                             add_cost_function, build_train_op, build_inference_op) and
 *                             voicepuppet/pixrefer/vgg_simple.py:96-162 (perceptual trunk)
 *   vp_adam_tf      replaces  tf.train.AdamOptimizer                    (pixrefer.py:398,405)
 *   vp_conv_* etc.  the single ops behind them (tf.layers.conv2d / conv2d_transpose /
 *                             batch_normalization: pixrefer.py:61-101), exported for parity tests
 *   vp_logmel_*     replaces  generator/generator.py:60-80              (DataGenerator.extract_mfcc)
 *   vp_bfmnet_*     replaces  voicepuppet/bfmnet/bfmnet.py:189-213,325-333 + tinynet.py:159-212
 *   vp_render_colors   replaces  utils/cython/mesh_core.h:63 _render_colors_core (mesh_core.cpp:169-231)
 *   vp_rasterize_triangles, vp_render_texture, vp_vertex_normals replace the rest of mesh_core.h:53-77 (_rasterize_triangles_core,
 *                             _render_texture_core, _get_normal_core: mesh_core.cpp:85-166, :234-333); vp_raster_interpolate and
 *                             vp_raster_vertex_visibility go with them
 *   vp_bfm_reconstruct replaces  utils/reconstruct_mesh.py:198-223 Reconstruction_rotation + infer_bfmvid.py:92-99
 *   vp_bfm_reconstruct_view replaces utils/reconstruct_mesh.py:172-194 Reconstruction + the packing of utils/bfm_visual.py:100-112 (view 0)
 *                             and voicepuppet/bfmnet/infer_bfmnet.py:212-216 (view 1)
 *   vp_sheet_tile_u8   replaces  utils/bfm_visual.py:125-128 (cvtColor + the numpy paste of a tile into big_img)
 *   vp_landmark_distance replaces nothing: the reference judges BFMNet by the montage alone (68-landmark distance, on the device)
 *   vp_bfmfit_*        replaces  infer_bfmvid.py:47-74 and datasets/make_data_from_GRID.py:193-214 (FaceReconModel.pb, a frozen TF1 ResNet) for the
 *                             identity, expression and pose of the 257 coefficients: a float64 fit to 68 landmarks, batched over frames;
 *                             vp_bfmfit_observe(_ex) / vp_bfmfit_appearance for texture and lighting: a float64 fit to the photo's pixels
 *   vp_puppet_*        replaces  infer_bfmvid.py:110-121, :223-224, :229-238 for the rows of many talkers (stream groups)
 *   vp_jpeg_*          replaces  infer_bfmvid.py:243-244 (cv2.imwrite per frame) with a baseline JPEG encode on the device
 *   vp_png_*           replaces  train_pixrefer.py:105-118 (five tf.summary.image calls: PNG through zlib on the host) with a PNG encode on the device
 *   vp_avimux_*        replaces  infer_bfmvid.py:245 (ffmpeg over the .jpg files and the wav) with Motion-JPEG + PCM AVI segments built on the device
 *   vp_jpegdec_*       replaces  generator/generator.py:956-1019 (cv2.imread per sample) and loader.py ImageLoader with a baseline JPEG decode on the device
 *   vp_pcmin_*         replaces  generator/loader.py:39-54 (WavLoader: scale, channel mean, resample_poly over a whole file) for live PCM
 *   vp_triptych_*      replaces  datasets/make_data_from_GRID.py:430-469 (step 5: binary_fill_holes, cv2.resize, erode, GaussianBlur, the paste and the
 *                             three panels of a training triptych) and :690-695 (step 6's layout with an alpha matte)
 *   vp_frame_metrics_* replaces  nothing: the reference has no image-quality measure (L1, PSNR and SSIM per frame pair, on the device)
 *   vp_keymatte_*      replaces  the matte that step 6 of datasets/make_data_from_GRID.py (:690-695) takes from its segmentation and matting
 *                             models, for footage in front of a PLAIN backdrop only: a colour key with an edge-aware clean-up, no network
 *   vp_matteclean_*    replaces  nothing: the reference pastes its matting network's output as it is (components that are not the subject,
 *                             holes in it); vp_key_foreground likewise: the reference trains on frame x matte, backdrop fringe included
 *   vp_mattesolve_*    replaces  datasets/make_data_from_GRID.py:654-672 (step 6's trimap from an erosion and a dilation of the mask, and
 *                             its matting network): a closed-form matting solve in the trimap's band, no network and no weights
 *
 * Conventions: every function returns 0 on success and a negative vp_status otherwise (never throws);
 * all tensor pointers are DEVICE pointers owned by the caller (NHWC, row-major); nothing is allocated
 * on the device by the library - workspace sizes are queried and the caller passes the buffer; every
 * launch goes to the hipStream_t given (passed as void*), no call synchronises.
 */
#ifndef VP_HIP_H_
#define VP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vp_status { VP_OK = 0, VP_ERR_ARG = -1, VP_ERR_HIP = -2, VP_ERR_WORKSPACE = -3, VP_ERR_STATE = -4 };
enum vp_dtype { VP_F32 = 0, VP_BF16 = 1 };
enum vp_act { VP_ACT_NONE = 0, VP_ACT_LRELU = 1, VP_ACT_RELU = 2, VP_ACT_TANH = 3, VP_ACT_SIGMOID = 4, VP_ACT_RELU6 = 5, VP_ACT_LEAKY = 6 };

int vp_version(void);
const char* vp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * PixReferNet step (pixrefer.py:356-438)
 * ---------------------------------------------------------------------------------------------- */
typedef struct vp_pixrefer_desc {
  int batch;        /* per-device batch N */
  int height;       /* square images, multiple of 256 */
  int ngf, ndf;     /* pixrefer.py:28-29 (64, 64) */
  int dtype;        /* vp_dtype of activations / MFMA operands; master weights, statistics, losses are f32 */
  int training;     /* 1: build_train_op graph (G + 3xD + VGG + losses + grads); 0: build_inference_op */
  float l1_weight;  /* pixrefer.py:30-31 */
  float gan_weight;
  int per_sample_bn; /* inference only: batch-norm statistics per sample (== running N frames through the
                        reference's batch-1 graph, infer_bfmvid.py:152,198, but batched on the device) */
  /* Schedule of a training plan, fixed at vp_pixrefer_create (no reference counterpart: the TF graph has one executor).  0 = default
   * in every field, so a zero-initialised tail keeps the shipped schedule; results are bit-identical under every setting.
   *   streams          0 / 4: the step is spread over the caller's stream + three of the executor's; 3: three in all (a host with a busy
   *                    stream of its own, vp_pixrefer_use_streams); 1: the executor creates no stream, everything runs on the caller's
   *   d_backward_fork  0: default (the discriminator-loss pass starts behind the generator-loss pass through D and the VGG trunk);
   *                    1 / 2 / 3: fork point 0 (at once) / 1 (behind the pass through D) / 2 (the default)
   *   d_beside_vgg     0 / 2: discriminator passes on the branch stream beside the VGG passes (default); 1: on the caller's stream */
  int streams;
  int d_backward_fork;
  int d_beside_vgg;
} vp_pixrefer_desc;

/* ABI rule for this descriptor (the precedent is utils/cython/mesh_core.h:53-77: explicit sizes, caller-owned buffers): the struct only
 * ever GROWS AT THE TAIL (rounds 1-4: the first 9 fields = 36 bytes; round 5 added the three schedule fields = 48 bytes), and every entry
 * point that takes it reads sizeof(vp_pixrefer_desc) bytes OF THE LIBRARY'S BUILD.  A binding that declares the struct itself (ctypes,
 * cgo, JNI) must check vp_pixrefer_desc_size() == its own sizeof at load time and refuse to run on a mismatch - a shorter struct would
 * be over-read (INTEGRATION.md B does; tests/test_host_logic.py executes that stub under AddressSanitizer). */
size_t vp_pixrefer_desc_size(void);

typedef struct vp_pixrefer vp_pixrefer_t;

/* Parameter manifest: TF variable names -> offset/shape in the flat f32 arenas.
 * which: 0 = generator*, 1 = discriminator*, 2 = vgg_16 (conv1_1 .. conv3_3).
 * vp_pixrefer_param_info returns VP_OK and fills the outputs, or VP_ERR_ARG when index is past the end. */
size_t vp_pixrefer_param_count(const vp_pixrefer_desc* d, int which);
int vp_pixrefer_param_info(const vp_pixrefer_desc* d, int which, int index, char* name, int name_cap,
                           size_t* offset, int* ndim, int64_t shape[4]);

size_t vp_pixrefer_workspace_bytes(const vp_pixrefer_desc* d);
/* Host-only self-check of the plan a descriptor produces (no GPU needed): every buffer the kernels would be handed is a carved
 * region of sufficient size inside the workspace, regions do not overlap, parameter / packed-weight ranges lie inside their
 * arenas, split-K slabs fit the scratch.  VP_OK, VP_ERR_ARG (bad descriptor) or VP_ERR_STATE (vp_last_error names the breach).
 * Run under AddressSanitizer / UBSan by the `make host-asan` build of the host layer (tests/test_host_logic.py). */
int vp_pixrefer_validate_plan(const vp_pixrefer_desc* d);

/* params_* / grads_*: flat f32 device arenas laid out as the manifest says (grads may be NULL when
 * training == 0; params_d / params_vgg likewise). */
int vp_pixrefer_create(const vp_pixrefer_desc* d, void* workspace, size_t workspace_bytes,
                       float* params_g, float* params_d, const float* params_vgg,
                       float* grads_g, float* grads_d, void* stream, vp_pixrefer_t** out);
void vp_pixrefer_destroy(vp_pixrefer_t* h);

/* Call after the f32 master parameters changed: _params_changed after the host wrote any arena (checkpoint load, initialisation:
 * all three nets are re-packed), _optimizer_stepped after vp_adam_tf on generator* / discriminator* (the frozen vgg_16 trunk -
 * restored from a checkpoint, never an optimiser variable: pixrefer.py:325-327, 396-407 - keeps its packed weights). */
int vp_pixrefer_params_changed(vp_pixrefer_t* h);
int vp_pixrefer_optimizer_stepped(vp_pixrefer_t* h);

/* inputs [N,H,H,6], fg_inputs [N,H,H,6] (inference: only channels 0:3 are read), targets [N,H,H,3],
 * masks [N,H,H,3] (training only) - float32 in [0,1] exactly as PixReferDataGenerator yields them
 * (generator.py:1011-1019).  Runs the generator, the composite, and when training the three
 * discriminator applications, the VGG trunk and all losses. */
int vp_pixrefer_forward(vp_pixrefer_t* h, const float* inputs, const float* fg_inputs,
                        const float* targets, const float* masks, void* stream);

/* The inference graph as infer_bfmvid.py:202-205 feeds it: fg_inputs3 [N,H,H,3] (build_inference_op reads fg_inputs[..., :3] only,
 * pixrefer.py:281).  Inference plans only (VP_ERR_STATE on a training plan, whose graph reads channels 3:6 too). */
int vp_pixrefer_forward_fg3(vp_pixrefer_t* h, const float* inputs, const float* fg_inputs3, const float* targets, void* stream);

/* Both gradient sets from the forward just run: d(Discrim_loss)/d(discriminator*) -> grads_d,
 * d(Gen_loss)/d(generator*) -> grads_g (pixrefer.py:396-407; pre-update weights for both). */
int vp_pixrefer_backward(vp_pixrefer_t* h, void* stream);
/* vp_pixrefer_backward + both tf.train.AdamOptimizer updates (vp_adam_tf on generator* and discriminator*) + the weight re-pack
 * the next forward would do, as ONE call: every range of an arena is updated as soon as its gradients are final, on the side /
 * branch streams under the rest of the backward pass.  m / v: Adam slot arenas (same layout as the parameter arenas);
 * step_t: 1-based Adam step of each optimiser.  Parameters after the call are bit-identical to the three separate calls.
 * Single-GPU steps only: a data-parallel host must all-reduce the gradients first (vp_pixrefer_backward_g_stage). */
int vp_pixrefer_backward_update(vp_pixrefer_t* h, float* m_g, float* v_g, float* m_d, float* v_d, int step_t_g, int step_t_d,
                                float lr, float beta1, float beta2, float eps, void* stream);

/* The two halves of vp_pixrefer_backward, so a data-parallel host can start the all-reduce of the
 * discriminator gradients while the generator backward runs. */
int vp_pixrefer_backward_d(vp_pixrefer_t* h, void* stream);
int vp_pixrefer_backward_g(vp_pixrefer_t* h, void* stream);
/* vp_pixrefer_backward runs the two (independent) halves CONCURRENTLY: the discriminator-loss pass on a HIP stream the handle
 * owns, forked from and joined into `stream` with events (no host blocking; bit-identical results).  The same for a host with
 * work of its own in between: _fork schedules the discriminator-loss pass (it starts inside stage 0 of the generator backward,
 * behind the generator-loss pass through the discriminator - or at once with vp_pixrefer_set_option(h, "d_backward_fork", 0)), _join makes `stream`
 * wait for it; grads_d is final after the join, which may come after any stage (the later, the more of the pass is hidden).  (vp_pixrefer_desc::streams = 1: both run
 * on `stream`, one after the other.) */
int vp_pixrefer_backward_d_fork(vp_pixrefer_t* h, void* stream);
int vp_pixrefer_backward_d_join(vp_pixrefer_t* h, void* stream);
/* The executor's own side stream (hipStream_t), for a data-parallel host that issues its collectives there instead of on one more
 * stream of its own (the device has few hardware queues; streams beyond them share one).  Work the host enqueues on it runs behind the
 * discriminator-loss pass of the step.  NULL if the plan runs on a single stream (vp_pixrefer_desc::streams = 1). */
void* vp_pixrefer_side_stream(vp_pixrefer_t* h);
/* The executor's three extra HIP streams are process-wide (one device per process), created once - by this call, or by the first
 * training plan - and shared by every plan of the process; they are never destroyed.  A host that also creates an RCCL communicator (or
 * any other busy stream) calls this FIRST: streams created behind other streams get the HIP runtime's leftover hardware queues and the
 * step runs 8 % (32 frames) to 30 % (4 frames) slow (scripts/exp_dp_order.py).  No counterpart in the reference (tf.Session owns its
 * executor, train_pixrefer.py:34). */
int vp_reserve_streams(void);
/* The fourth of those streams, for a host with ONE busy stream of its own (an input prefetcher: generator/device_pipeline.py
 * FramePrefetcher) whose plans keep to three (vp_pixrefer_use_streams(h, 3)): a stream the host created itself would be the process's
 * fifth and share a hardware queue (the PCIe-inclusive step: 9.2 ms instead of 7.4).  NULL on error (vp_last_error). */
void* vp_host_stream(void);
/* Streams a training step is spread over: 4 (default) or 3.  A host that runs a busy stream of its own beside the step (an input
 * prefetcher) asks for 3: the device has few hardware queues, a fifth busy stream shares one with an executor stream. */
int vp_pixrefer_use_streams(vp_pixrefer_t* h, int n);
/* Schedule options of ONE plan (no reference counterpart: the TF graph has one executor): "overlap" 0 / 1 (the whole step on `stream`
 * / spread over the executor's streams, default 1), "d_backward_fork" 0..2 (where vp_pixrefer_backward starts the discriminator-loss
 * pass, default 2), "d_beside_vgg" 0 / 1 (default 1); and "store_first_raw" 0 / 1 (default 0): encoder_1 / encoder_fg_1 / discriminator
 * layer_1 of a bf16 plan write their consumers' activations from the conv epilogue and skip the raw output nobody reads - 1 stores it
 * too (vp_pixrefer_tensor refuses "g/encoder_1" ... otherwise).  The option also governs the full-resolution outputs of VGG conv1_2 /
 * conv2_2: with 0 the fake half of a bf16 step on the overlapped schedule writes only their 2x2 max pool and one byte per pooled element
 * for the pool's backward pass ("v/conv1/conv1_2" and "v/conv2/conv2_2" are refused the same way); 1 stores them as before.  Per handle: two plans in one process do not change each other's schedule; the
 * initial values come from the descriptor (vp_pixrefer_desc::streams / d_backward_fork / d_beside_vgg).  Bit-identical results under
 * every setting. */
int vp_pixrefer_set_option(vp_pixrefer_t* h, const char* key, int value);
/* Round 6 keys: "bwd_sums_in_epilogue" 0 / 1 (default 1): the two sums of a batch-norm backward pass (sum dz, sum dz * zhat) come from the
 * epilogue of the launch that completes the tensor's gradient instead of a pass of their own over y and dz (same values up to the order of
 * float32 partial sums); "vgg_real_fork" k (default 3): the VGG pass of the real half starts on the side stream in front of generator layer
 * k (TF scope order; 0 = right behind the input packing).  vp_pixrefer_counter: "bwd_sums_launches" = launches since create that carried
 * such sums; "pool_codes_written" = 1 when the last forward pass wrote the VGG pool codes in place of the full-resolution conv1_2 /
 * conv2_2 outputs of the fake half, else 0; "pool_bwd_fused" = 1 when the last backward pass left the VGG pools' gradients to the loader
 * of the conv_c64 backward-data launches below them (vp_tune "pool_bwd_fused"; "v/conv1/conv1_2:dy" / "v/conv2/conv2_2:dy" are then
 * written out when vp_pixrefer_tensor asks for them), else 0 (-1: unknown key); for tests. */
long long vp_pixrefer_counter(vp_pixrefer_t* h, const char* key);
/* Node values PixReferNet.execute hands to a caller, formed on the device from the last forward pass into `dst` (device memory,
 * N * H * H * 3 elements): what = 0 Outputs (float32, (x + 1) / 2: pixrefer.py:424 / :380), 1 the same as uint8 frames (clamp, * 255,
 * truncate: the bytes infer_bfmvid.py:243 writes), 2 Alphas (float32, three channels: pixrefer.py:284), 3 Outputs_FG as this plan's
 * graph defines it (build_inference_op: ((Outputs_FG + Alphas - 1) + 1) / 2, pixrefer.py:436; build_train_op: the tensor itself). */
int vp_pixrefer_fetch(vp_pixrefer_t* h, int what, void* dst, void* stream);
/* The same pass in vp_pixrefer_backward_g_stages() = 3 consecutive stages (stage < 0: all).  After stage s a contiguous
 * range of the generator gradient arena is final (0: from generator/merged_decoder_5 to the end; 1: from
 * generator/merged_encoder_2 up to merged_decoder_5; 2: the rest), so a data-parallel host can start that bucket's
 * all-reduce while the next stage computes.
 * STREAM-ORDER CONTRACT for a host that hands an arena range to another stream (a collective): the executor runs parts of a stage
 * on HIP streams of its own, but before vp_pixrefer_backward_g_stage / vp_pixrefer_backward_d_join return they have made `stream`
 * wait (hipStreamWaitEvent) for every kernel that writes the range the call completes.  An event recorded on `stream` right after
 * the call therefore covers the whole range; the collective's stream must wait for THAT event (voicepuppet_amd/parallel.py
 * GradExchange does) - it must not read the arena on the strength of host-side ordering alone. */
int vp_pixrefer_backward_g_stages(void);
int vp_pixrefer_backward_g_stage(vp_pixrefer_t* h, int stage, void* stream);
/* Data parallel: tf.train.AdamOptimizer + weight re-pack of ONE gradient bucket on `stream`, for a host that has just all-reduced
 * it there: which = 0 generator (bucket = the stage that completed it), which = 1 discriminator (bucket 0).  `stream` must be
 * ordered behind that stage (see the contract above).  Bit-identical to vp_adam_tf over the whole arena; after the four buckets of
 * a step the packed weights are current (the next forward re-packs nothing). */
int vp_pixrefer_update_bucket(vp_pixrefer_t* h, int which, int bucket, float* m, float* v, int step_t, float lr, float beta1,
                              float beta2, float eps, void* stream);

/* Named device buffers ("nodes" of pixrefer.py:356-438 and every intermediate):
 *   "Outputs_raw" [N,H,H,3] f32 in [-1,1], "Outputs_FG" [N,H,H,3] f32, "gen_out4" [N,H,H,4] f32,
 *   "Predict" [2,N,h,h] f32 (real, fake), "losses" [8] f32 = {Discrim_loss, Gen_loss_GAN, Gen_loss_L1,
 *   Gen_loss, Perceptual_loss}, "g/<scope>" raw conv outputs, "g/<scope>:dy" their gradients, ...
 * dtype receives the vp_dtype of the buffer. */
int vp_pixrefer_tensor(vp_pixrefer_t* h, const char* name, void** ptr, int64_t shape[4], int* dtype);

/* Per-launch timing of the conv kernels with HIP events on the launch stream (bench.py roofline).
 * vp_profile_collect: JSON array [{name, calls, ms, flops, bytes}] since the last collect; call after
 * synchronising the stream; returns the bytes needed (including the terminator). */
int vp_profile_enable(int on);
size_t vp_profile_collect(char* json, size_t cap);

/* Input pipeline on the device.  Replaces the per-sample host work of PixReferDataGenerator.iterator (generator/generator.py:
 * 956-1019: BGR->RGB, split of the S x 3S triptych into target | 3-D face | matte, random square crop, cv2.resize back to S x S,
 * the 6-channel packing of (example, current) and fg = target * matte).  example_frames / current_frames: [n][S][3S][3] uint8
 * exactly as cv2.imread decodes the training jpgs; crops: [n][2][3] int32 = (rx rows, ry columns, rsize) for the example and the
 * current frame, 0 <= rx, ry and rx + rsize, ry + rsize <= S (drawn by the caller as generator.py:975-977, 994-996); outputs:
 * the four float32 tensors vp_pixrefer_forward takes.  All pointers are device memory; crop values are NOT range-checked. */
int vp_pixrefer_pack_frames(const unsigned char* example_frames, const unsigned char* current_frames, const int* crops,
                            int n, int img_size, float* inputs, float* fg_inputs, float* targets, float* masks, void* stream);

/* Kernel-selection knobs for tests and experiments (they choose between kernels that compute the same result); plans made AFTER
 * the call see the new value.  Keys: "patch_tiles" (bit 0 / 1 / 2: allow the 256- / 128- / 64-row tiles of the stride-1 patch
 * kernel, default 7), "patch_min_blocks" (smallest grid that runs on it, default 192 since round 6 - 384 before; < 0: back to the default), "patch_small_tiles" (bit 0: 16x16-pixel
 * tiles for the 128- / 64-row variants, bit 1: 8x16 for the 256-row variant - two blocks per CU; default 3), "patch_long_k_on_256"
 * (default 1: >= 512-channel layers with K >= 4096 stay on the wave-specialised 256x256 tile - float32 plans; bf16 plans: "patch4"), "c64" / "dc64" (default 1: the
 * register-resident-weights kernels conv_c64.hip / conv_dc64.hip - "dc64" also the forward form conv_dc256_kernel; 0: the patch kernels
 * those layers ran on before), "s2c64" (smallest launch, in 4 x 16-pixel tiles, of the 64 -> 128 stride-2 convolutions that runs on
 * conv_s2c64.hip: default 512, 0 = never), "s2c64_pair" (default 1: its two-output backward-data form for merged2_decoder_2), "patch4"
 * (default 1: 4x4 stride-1 layers on the unrolled patch kernel with 16 tap steps), "bfm_dwproj" (default 1: BFMNet's depthwise + projection
 * in one kernel; read at every forward call), "pool_bwd_fused" (default 1: where the forward pass wrote VGG pool codes and the backward-data
 * launch of conv1_2 / conv2_2 is planned on conv_c64.hip, that launch reads the pool's gradient and codes and expands them in its loader -
 * no pool-backward launch, no full-resolution gradient in memory - conv1_2 always, conv2_2 where its launch has at least 4096 tiles of 4 x 16
 * pixels, 16 frames at 256 x 256; 0: vp_maxpool2x2_bwd_code's kernel writes it out; 2 / 3 / 4: conv1_2 only / conv2_2 only / both at every size).  No counterpart in the reference.  (The step executor's schedule is per plan: vp_pixrefer_desc / vp_pixrefer_set_option.) */
int vp_tune(const char* key, int value);
/* Round-6 plan heuristics: "igemm_small_grid" (default 128: a launch whose 128 x 128 tiling has at most that many blocks per class takes the
 * 64-row x 128-pixel tile - twice the blocks; 0: off), "igemm_splitk_target" (default 64, rounds 2-5: 128: resident blocks a K split aims at;
 * < 0: back to the default); "thin_blocks_cout8" / "thin_blocks_dcout8" / "thin_blocks_cout4" / "thin_blocks_cin8" (defaults 1024 / 512 /
 * 512 / 512: grid caps of the persistent thin-layer kernels conv3x3_cout8_tile / deconv_cout8_tile / deconv_cout4_tile / conv_cin8;
 * values <= 0 are ignored); "cout1_bwd" (default 256: most blocks per batch-norm group of the one-output-channel backward-data kernel
 * conv_cout1.hip - the discriminator's layer_5 -, 0: that layer's backward passes on the generic kernels, < 0: back to the default), "cout1_wgrad_rows"
 * (default 512: most blocks = slabs of its weight-gradient kernel). */
/* Further keys: "smallp_max_pixels" (largest pixel count per parity class that runs on the few-pixel kernel conv_smallp.hip,
 * default 256, 0: off), "phase_marks" (1: the step executor records HIP events on the caller's stream at its phase boundaries).
 * vp_pixrefer_phase_ms: milliseconds between consecutive marks of the last step (synchronises on them): generator forward,
 * discriminator / VGG forward + losses, generator-loss pass through D and VGG + composite backward (including the host gap between
 * the forward and the backward call), generator backward stage 0, 1, 2, join of the discriminator-loss pass.  Returns the number written. */
int vp_pixrefer_phase_ms(vp_pixrefer_t* h, float* ms, int cap);
/* "phase_marks" = 2 adds a mark in front of every generator layer (forward: mark 8 + layer, backward on the caller's stream:
 * 32 + layer, layers in TF scope order); vp_pixrefer_mark_ms: milliseconds between two marks of the last step, -1 if not recorded. */
float vp_pixrefer_mark_ms(vp_pixrefer_t* h, int from, int to);

/* Data parallel, optional bf16 transport of a gradient bucket (the f32 arena stays the master copy): round n floats to bf16
 * (nearest even) into a communication buffer; after the bf16 all-reduce (sum) write them back as f32 times `scale` (= 1 / world).
 * src / dst float pointers 32-byte aligned, the bf16 buffer 16-byte aligned.  No counterpart in the reference (single device). */
int vp_grad_pack_bf16(const float* src, void* dst_bf16, size_t n, void* stream);
int vp_grad_unpack_bf16(const void* src_bf16, float* dst, size_t n, float scale, void* stream);

/* theta -= lr_t * m / (sqrt(v) + eps) with lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) (TF formulation) */
int vp_adam_tf(float* params, const float* grads, float* m, float* v, size_t n, int step_t,
               float lr, float beta1, float beta2, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Single ops (parity tests; same kernels the step uses).  x: NHWC in `dtype`.
 * in_scale/in_shift: optional per-channel deferred batch-norm affine of the producer, in_act applied
 * after it (pixrefer.py:182-186: act -> conv -> BN).  workspace: vp_conv_workspace_bytes().
 * ---------------------------------------------------------------------------------------------- */
typedef struct vp_conv_desc {
  int kind;          /* 0: conv2d HWIO (pixrefer.py:61-74, vgg_simple.py:138); 1: conv2d_transpose k4 s2 HWOI (pixrefer.py:85) */
  int n, h, w;       /* input size */
  int cin, cout;     /* cin % 8 == 0 and a power of two; any cout */
  int ksize, stride, pad;
  int dtype;
  int in_act;
  int out_act;       /* fwd only */
} vp_conv_desc;

size_t vp_conv_workspace_bytes(const vp_conv_desc* d);
/* y = out_act(conv(in_act(in_scale*x+in_shift), w) + bias); y in `dtype`, [n,ho,wo,cout] */
int vp_conv_fwd(const vp_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                const float* w, const float* bias, void* y, void* workspace, void* stream);
/* dx = d/d(in_act(...) input)  (i.e. w.r.t. the activated tensor the conv reads), [n,h,w,cin] in `dtype` */
int vp_conv_bwd_data(const vp_conv_desc* d, const void* dy, const float* w, void* dx, void* workspace, void* stream);
/* Backward-data of a 3x3 / stride-1 / pad-1 bf16 convolution with cin == cout in {64, 128} (h % 4 == 0, w % 16 == 0, h >= 16: conv_c64.hip) whose
 * output went through a 2x2 max pool - VGG conv1_2 / conv2_2 in the perceptual backward pass: dx [n,h,w,cin] = conv_bwd_data(unpool(dy_pool,
 * code)) * relu'(ref), with dy_pool [n,h/2,w/2,cout] the pool's gradient, code [n,h/2,w/2,cout] uint8 as for vp_maxpool2x2_bwd_code and ref
 * [n,h,w,cin] the stored relu output of the producer.  fused = 0: the unpooled gradient is written to the workspace (vp_maxpool2x2_bwd_code's
 * kernel) and read back by the convolution; fused = 1: the convolution's loader builds it in LDS from dy_pool and code.  Bit-identical. */
size_t vp_conv3x3_c64_bwd_data_pooled_workspace_bytes(const vp_conv_desc* d);
int vp_conv3x3_c64_bwd_data_pooled(const vp_conv_desc* d, const void* dy_pool, const unsigned char* code, const float* w, const void* ref,
                                   void* dx, void* workspace, int fused, void* stream);
/* dw in the TF layout of `kind`, f32 */
int vp_conv_bwd_weight(const vp_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                       const void* dy, float* dw, void* workspace, void* stream);

/* training-mode batch norm statistics (pixrefer.py:99-101): y [pixels, c] -> scale/shift (z = scale*y+shift),
 * mean, rstd; biased variance, eps inside the sqrt.  workspace: vp_bn_workspace_bytes(). */
size_t vp_bn_workspace_bytes(int pixels, int c, int dtype);
int vp_bn_stats(const void* y, int pixels, int c, int dtype, const float* gamma, const float* beta, float eps,
                float* scale, float* shift, float* mean, float* rstd, void* workspace, void* stream);
/* dy = BN backward of dz (in place allowed), dgamma, dbeta */
int vp_bn_bwd(const void* y, const void* dz, void* dy, int pixels, int c, int dtype, const float* gamma,
              const float* mean, const float* rstd, float* dgamma, float* dbeta, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Audio front-end (f32).
 * vp_logmel_*  : DataGenerator.extract_mfcc (generator/generator.py:60-80): Hann STFT -> |.| -> HTK mel -> log(.+1e-6)
 * vp_bfmnet_*  : BFMNet.build_inference_op (voicepuppet/bfmnet/bfmnet.py:325-333 -> 189-213) with MfccNet
 *                (tinynet.py:159-212) in inference mode; parameters by TF variable name (vp_bfmnet_param_info).
 * ---------------------------------------------------------------------------------------------- */
typedef struct vp_logmel_desc {
  int sample_rate, num_mel_bins, win_length, hop_step, fft_length;   /* config/params.yml:16-21; win == fft */
  float lower_hz, upper_hz;                                          /* 80, 7600 (generator.py:68) */
  int batch, samples;                                                /* pcm [batch, samples] */
} vp_logmel_desc;
typedef struct vp_logmel vp_logmel_t;
size_t vp_logmel_workspace_bytes(const vp_logmel_desc* d);
int vp_logmel_frames(const vp_logmel_desc* d);                       /* 1 + (samples - win)/hop */
int vp_logmel_create(const vp_logmel_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_logmel_t** out);
void vp_logmel_destroy(vp_logmel_t* h);
/* pcm [batch, samples] f32 in [-1,1] -> out [batch, frames, num_mel_bins] f32 */
int vp_logmel_forward(vp_logmel_t* h, const float* pcm, float* out, void* stream);

typedef struct vp_bfmnet_desc {
  int batch;          /* clips */
  int frames;         /* T video frames per clip; the mel input has 5*T frames (frame_mfcc_scale, generator.py:46-52) */
  int num_mel_bins;   /* 80 */
  int trunk_dtype;    /* VP_F32 (parity path: coefficients 1e-5 vs the float64 oracle) or VP_BF16 (opt-in, 2x the rate): the 6x-expanded
                         tensors and the 1x1-conv operands of MfccNet in bf16, f32 accumulation / residual stream / depthwise /
                         pooling / head; trunk features within 4e-2 rel-L2 of the oracle (tests/test_gpu_audio.py) */
} vp_bfmnet_desc;
typedef struct vp_bfmnet vp_bfmnet_t;
size_t vp_bfmnet_param_count(void);
int vp_bfmnet_param_info(int index, char* name, int name_cap, size_t* offset, int* ndim, int64_t shape[4]);
size_t vp_bfmnet_workspace_bytes(const vp_bfmnet_desc* d);
int vp_bfmnet_create(const vp_bfmnet_desc* d, void* workspace, size_t workspace_bytes, const float* params,
                     void* stream, vp_bfmnet_t** out);
void vp_bfmnet_destroy(vp_bfmnet_t* h);
int vp_bfmnet_params_changed(vp_bfmnet_t* h);
/* ears [B,T,1], mfccs [B,5T,80], seq_len [B] (int32) -> BFMCoeffDecoder [B,T,64]; all device pointers */
int vp_bfmnet_forward(vp_bfmnet_t* h, const float* ears, const float* mfccs, const int* seq_len, float* out, void* stream);
/* Opt-in: the reference's BFMCoeffDecoder applies tf.nn.dropout(keep_prob = 0.75) behind both hidden dense layers unconditionally,
 * i.e. also at inference (voicepuppet/bfmnet/bfmnet.py:114,116: that class's drop_rate is never zeroed).  The default forward omits
 * both (deterministic: the expectation of the reference's output).  With masks set - mask0 [B*T,128], mask1 [B*T,64], device f32,
 * entries 0 or 1 / keep_prob, owned by the caller until cleared with NULLs - every following forward multiplies the two hidden
 * activations by them: one SAMPLE of the reference's inference output for that draw. */
int vp_bfmnet_set_decoder_dropout(vp_bfmnet_t* h, const float* mask0, const float* mask1);
/* "MfccEncoder" [B,T,256], "RNNModule" [B,T,256] of the last forward */
int vp_bfmnet_tensor(vp_bfmnet_t* h, const char* name, void** ptr, int64_t shape[4]);

/* ------------------------------------------------------------------------------------------------
 * Streaming BFMNet inference (one session per handle): PCM goes in by chunks of any size, the 64 coefficients of a video frame come
 * out as soon as the frame's receptive field has arrived - the same frames, with the same values up to kernel choice, as
 * vp_logmel_forward + vp_bfmnet_forward on the whole clip padded as infer_bfmvid.py:162-167 pads it (pad_len = 1 + N / 640 frames).
 *   - Every mel frame (512 samples, hop 128) is computed once, by the log-mel kernel of vp_logmel_forward, into a device history.
 *   - Every MfccNet convolution has time stride 1, so a frame's pooled encoding depends on a bounded window of mel rows: left_mel /
 *     right_mel (vp_bfmstream_context, derived from the layer table).  A push recomputes the trunk on a window of
 *     T_win = max_chunk_frames + left + right frames around the frames it emits; the GRU runs over the emitted frames only, its state
 *     carried across pushes (bit-identical to one uncut run).
 *   - Emission counts follow from sample counts alone: the host never waits on the device inside push / finish.
 *   - A session is a stream group of one slot (vp_bfmstream_group_*, below): the same executor, its workspace that group's.
 * 640 samples per video frame, 5 mel frames per video frame (config/params.yml: 16 kHz, 25 frames/s, hop 128, window 512).
 * ---------------------------------------------------------------------------------------------- */
typedef struct vp_bfmstream_desc {
  int struct_bytes;       /* sizeof(vp_bfmstream_desc) of the caller's build: must equal vp_bfmstream_desc_size() */
  int max_chunk_frames;   /* most frames one window emits (1 .. 1024); a push that makes more ready runs several windows */
  int num_mel_bins;       /* 80 */
  int trunk_dtype;        /* VP_F32 or VP_BF16, as vp_bfmnet_desc */
  int sample_rate;        /* mel matrix: 16000 */
  float lower_hz, upper_hz;   /* 80, 7600 */
} vp_bfmstream_desc;
/* Same ABI rule as vp_pixrefer_desc: the struct only grows at the tail; entry points refuse a descriptor whose struct_bytes differs */
size_t vp_bfmstream_desc_size(void);
typedef struct vp_bfmstream vp_bfmstream_t;
/* Host only.  Receptive field of one pooled frame in mel rows (left_mel, right_mel), the same in video frames, and the window plan's
 * frames.  Any output pointer may be NULL.  VP_ERR_ARG on a bad descriptor. */
int vp_bfmstream_context(const vp_bfmstream_desc* d, int* left_mel, int* right_mel, int* left_frames, int* right_frames, int* window_frames);
/* Host only.  Frames emitted in all once `samples` samples have been pushed (finished = 0), or after finish (finished = 1: pad_len) */
long long vp_bfmstream_frames_after(const vp_bfmstream_desc* d, long long samples, int finished);
size_t vp_bfmstream_workspace_bytes(const vp_bfmstream_desc* d);
/* params: the vp_bfmnet_* parameter arena (vp_bfmnet_param_info), device, read at every window; vp_bfmstream_params_changed after
 * writing it */
int vp_bfmstream_create(const vp_bfmstream_desc* d, void* workspace, size_t workspace_bytes, const float* params, void* stream,
                        vp_bfmstream_t** out);
void vp_bfmstream_destroy(vp_bfmstream_t* h);
int vp_bfmstream_params_changed(vp_bfmstream_t* h);
/* back to an empty session (no samples, zero GRU state), enqueued on stream */
int vp_bfmstream_reset(vp_bfmstream_t* h, void* stream);
/* Host only: frames the next push of n_new_samples emits (vp_bfmstream_ready) / finish emits (vp_bfmstream_ready_finish) */
int vp_bfmstream_ready(const vp_bfmstream_t* h, long long n_new_samples);
int vp_bfmstream_ready_finish(const vp_bfmstream_t* h);
/* pcm [n] f32 device, any n; ears [k,1] and coeff_out [k,64] device with k = vp_bfmstream_ready(h, n) (may be NULL when k = 0) */
int vp_bfmstream_push(vp_bfmstream_t* h, const float* pcm, long long n, const float* ears, float* coeff_out, void* stream);
/* end of the clip: zero-pads as prepare_pcm does and emits the last k = vp_bfmstream_ready_finish(h) frames; the session then takes
 * no more pushes until vp_bfmstream_reset */
int vp_bfmstream_finish(vp_bfmstream_t* h, const float* ears, float* coeff_out, void* stream);
/* "mel" (the mel history ring, [rows][num_mel_bins]; row r of the clip sits at r % rows) */
int vp_bfmstream_tensor(vp_bfmstream_t* h, const char* name, void** ptr, int64_t shape[4]);
/* ------------------------------------------------------------------------------------------------
 * Streaming groups: `slots` independent vp_bfmstream sessions behind one handle, for serving many talkers from one GPU.  A group push
 * advances any subset of the slots by any number of samples each and runs ONE kernel chain per round for all of them: a ragged
 * log-mel launch into each slot's mel ring, a ragged window gather, the MfccNet trunk on a plan of batch A (the active slots, rounded up
 * to a bucket 1, 2, 4, .., slots), the stateful GRU with one block per slot, the decoder and one scatter into the packed output.  A slot
 * with more than max_chunk_frames ready runs further rounds, with the other slots that still have frames.
 *   - Each slot's coefficients are bit-identical to a vp_bfmstream with the same max_chunk_frames and trunk_dtype fed the same chunks.
 *     A vp_bfmstream is a group of one slot, so this holds by construction; the bucket plans of more slots reduce every row as the
 *     batch-1 window plan does (each GEMM's tile and K split pinned to that plan's).
 *   - A slot that finishes a clip shorter than T_win runs its last frames alone on an exact-size plan, one slot after the other: the
 *     slow path of short clips.
 *   - Emission counts follow from sample counts alone (vp_bfmstream_group_ready); a push never waits on the device.
 * ---------------------------------------------------------------------------------------------- */
#define VP_BFMSTREAM_GROUP_MAX_SLOTS 128
typedef struct vp_bfmstream_group_desc {
  int struct_bytes;       /* sizeof(vp_bfmstream_group_desc) of the caller's build: must equal vp_bfmstream_group_desc_size() */
  int slots;              /* 1 .. VP_BFMSTREAM_GROUP_MAX_SLOTS */
  int max_chunk_frames;   /* per slot and round, as vp_bfmstream_desc */
  int num_mel_bins;       /* 80 */
  int trunk_dtype;        /* VP_F32 or VP_BF16 */
  int sample_rate;        /* 16000 */
  float lower_hz, upper_hz;   /* 80, 7600 */
} vp_bfmstream_group_desc;
/* Same ABI rule as vp_bfmstream_desc (the struct only grows at the tail; a wrong struct_bytes is refused) */
size_t vp_bfmstream_group_desc_size(void);
typedef struct vp_bfmstream_group vp_bfmstream_group_t;
/* 0 on a refused descriptor (vp_last_error says why): bad struct_bytes / slots / stream fields, or a slots x max_chunk_frames whose
 * batch-`slots` plan would exceed the 32-bit lane offsets of the kernels the one-stream plan runs (launch_dwproj, the GEMM loader) */
size_t vp_bfmstream_group_workspace_bytes(const vp_bfmstream_group_desc* d);
/* Host only (tests): GEMM `gemm` of bucket plan `bucket` (0: batch 1, 1: batch 2, ..): info = {batch, tile cfg, K splits, kernel,
 * pixels, input channels, output channels, bf16 operands} */
int vp_bfmstream_group_plan_info(const vp_bfmstream_group_desc* d, int bucket, int gemm, int info[8]);
int vp_bfmstream_group_create(const vp_bfmstream_group_desc* d, void* workspace, size_t workspace_bytes, const float* params, void* stream,
                              vp_bfmstream_group_t** out);
void vp_bfmstream_group_destroy(vp_bfmstream_group_t* h);
int vp_bfmstream_group_params_changed(vp_bfmstream_group_t* h);
/* slot back to an empty session (a new clip); the other slots are untouched */
int vp_bfmstream_group_reset_slot(vp_bfmstream_group_t* h, int slot, void* stream);
/* Host only: frames k[s] (k may be NULL) the push of n[s] new samples per slot emits, finish[s] != 0 ending slot s's clip after them
 * (finish may be NULL); returns the sum, or -1 on a bad argument (n[s] < 0, samples or finish for a finished slot) */
long long vp_bfmstream_group_ready(const vp_bfmstream_group_t* h, const long long* n, const int* finish, int* k);
/* pcm: device f32, the slots' new samples packed in slot order (n[s] each; n / finish are host arrays of `slots` entries, finish may be
 * NULL).  finish[s]: append n[s] samples, then end slot s's clip as vp_bfmstream_finish does.  ears [K,1] / coeff_out [K,64]: device,
 * K = vp_bfmstream_group_ready(...), rows packed in slot order (may be NULL when K = 0) */
int vp_bfmstream_group_push(vp_bfmstream_group_t* h, const float* pcm, const long long* n, const int* finish, const float* ears, float* coeff_out,
                            void* stream);
/* "mel": the slots' mel rings [slots][rows][num_mel_bins]; mel frame r of slot s's clip sits at row r % rows */
int vp_bfmstream_group_tensor(vp_bfmstream_group_t* h, const char* name, void** ptr, int64_t shape[4]);
/* The stateful GRU step loop on its own (testing / other drivers): rows [t0, t0 + n) of each of b sequences of t rows, state in / out
 * in hstate [b][256] (zeros = a fresh sequence).  Same layout as vp_gru_seq. */
int vp_gru_seq_state(const float* xg, const float* xc, const float* whg, const float* whc, float* hstate, float* out, int b, int t, int t0,
                     int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Single pointwise / audio ops of the two executors (the entry-point list of SURVEY.md 8b), for parity tests and reuse.
 *   vp_maxpool2x2_*      slim max_pool2d 2x2/2 of vgg_simple.py:141,146 (NHWC).  bwd goes through the pool AND the ReLU of the conv
 *                        that produced x (x is stored post-relu): the gradient lands on the FIRST maximum of a window if it is > 0
 *   vp_maxpool2x2_bwd_code  the same from one byte per pooled element instead of x (code [n][h/2][w/2][c], uint8: 0 = the window maximum
 *                        is <= 0, no gradient; 1 + k = position k of the window in the order (0,0), (0,1), (1,0), (1,1) is its first
 *                        maximum): what a training step's fused-pool conv epilogues record in place of the full-resolution tensor
 *   vp_composite_fwd     pixrefer.py:279-290 inference compositing: out4 = tanh(gen_out4), alpha = (out4[3]+1)/2,
 *                        outputs = rgb*alpha + (2*targets-1)*(1-alpha), outputs_fg = rgb*alpha + alpha - 1   (all float32)
 *   vp_gan_loss          pixrefer.py:334-347: logits [3][m] = D(real1) | D(real2) | D(fake) -> predict [2][m], losses[0] = Discrim_loss,
 *                        losses[1] = Gen_loss_GAN, and the loss seeds w.r.t. the logits ([3][m][8] / [m][8] of dtype, channel 0)
 *   vp_dwconv7x3_bn_act  tinynet.py depthwise [7,3] stride 1 'same' + folded BatchNorm (bias) + relu6; w [21][c], float32 NHWC
 *   vp_dwconv7x3_bn_act_t  the same with x / y stored as dtype (VP_F32: the column-pair kernel; VP_BF16: the bf16 trunk's kernel, f32 sums)
 *   vp_conv_first_fwd    tinynet.py:168 stem: conv [9,5] stride [1,2] 'same' of x [b][h][w] (one channel) + folded bias + relu;
 *                        w [45][cout] (row 5 kh + kw), y [b][h][ceil(w/2)][cout], float32
 *   vp_dwproj_fwd        the second half of an inverted-residual block in ONE kernel (bfm_dwproj.hip), float32: depthwise [7,3] 'same'
 *                        + folded bias + relu6 of ex [b][h][w][ce], then the 1x1 projection w_proj [ce][cout] + b_proj into
 *                        y [b][h][w][cout] (add != 0: added to what y holds - the residual).  w_dw [21][ce], b_dw [ce].  The projection
 *                        weights are packed as the forward plan packs them, into the workspace (vp_dwproj_workspace_bytes; 0 for a
 *                        channel count the kernel never takes).  VP_ERR_ARG, before any launch, for a (w, ce, cout) without a kernel
 *                        (w / cout pairs of MfccNet; ce a multiple of 16) or an expanded tensor of 0xF0000000 bytes or more
 *   vp_maxpool_hw        tf.layers.max_pooling2d(k, s, 'same') (tinynet.py:178-190, bfmnet.py:35); output ceil(h/sh) x ceil(w/sw)
 *   vp_gru_seq           tf.contrib.rnn.GRUCell under dynamic_rnn (bfmnet.py:53-61), 256 units: xg [b,t,512] / xc [b,t,256] are the input
 *                        projections (+ biases), whg [256][512] / whc [256][256] the recurrent halves of gates / candidate kernels
 * ---------------------------------------------------------------------------------------------- */
int vp_maxpool2x2_fwd(const void* x, void* y, int n, int h, int w, int c, int dtype, void* stream);
int vp_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int dtype, void* stream);
int vp_maxpool2x2_bwd_code(const void* code, const void* dy, void* dx, int n, int h, int w, int c, int dtype, void* stream);
int vp_composite_fwd(const float* gen_out4, const float* targets, float* out4, float* outputs, float* outputs_fg, int n, int hw,
                     void* stream);
int vp_gan_loss(const float* logits, void* seed_d, void* seed_g, float* predict, float* losses, int m, float gan_weight, int dtype,
                void* stream);

/* ------------------------------------------------------------------------------------------------
 * The PixReferNet training step's pointwise kernels one at a time (csrc/pointwise.hip; tests/test_gpu_pixrefer_pointwise_ops.py): an
 * argument check and the launcher the step executor calls.  Tensors are [groups * pixels_per_group][c] in `dtype`; per-group vectors are
 * [groups][c] float32; c is a multiple of the element vector (4 for VP_F32, 8 for VP_BF16); at most 1024 groups.  Every entry point returns VP_ERR_ARG before
 * anything is enqueued for a null required pointer, a non-positive size or such a channel count; the two-pass batch-norm paths and
 * vp_colsum_groups also for 256 % (c / vector) != 0 (the reduce kernel's thread layout).
 *   vp_bn_groups_fwd       training-mode batch norm per group (pixrefer.py:99-101): scale / shift (z = scale * y + shift), mean, rstd, and
 *                          optionally lrelu(z) / relu(z) (either may be null).  path: VP_BN_PATH_PLANNER takes the step planner's rule
 *                          (one launch up to 2048 pixels per group), _TWO_PASS forces reduce + finalize (+ vp_act_apply's kernel),
 *                          _ONE_LAUNCH forces the small-tensor kernel.  workspace: vp_bn_groups_workspace_bytes() (unused in one launch)
 *   vp_bn_groups_bwd       dy = gamma rstd (dz - c1 - zhat c2) (dy may alias dz), c1 / c2 [groups][c], dgamma / dbeta [c] summed over the
 *                          groups (accumulate != 0: added to what they hold), dbias_zero [c] (may be null) set to 0.  Same path argument
 *   vp_bn_groups_bwd_tail  the same from caller-made partial rows [groups][nchunk][2][c] of doubles: (sum dz, sum dz zhat), or with
 *                          raw = 1 the raw moments (sum dz, sum dz y) a convolution epilogue leaves
 *   vp_colsum_groups       out[0:creal] (+)= sum over all pixels of x[.][0:creal], creal <= c (bias gradients of the BN-free layers)
 *   vp_act_apply           out_lrelu / out_relu (either may be null) = act(scale[g] * y + shift[g]); scale and shift both null: act(y)
 *   vp_relu_bwd            d[i] = y[i] > 0 ? d[i] : 0 in place, n elements
 *   vp_tap_gather          discriminator layer_5 as a GEMM over taps, gather half: y[n][i][j] = bias[0] + sum over (kh, kw) inside the image
 *                          of s[n][i + kh - pad][j + kw - pad][kh * ksize + kw], s [n][hin][win][16] float32, ksize <= 4
 *   vp_tap_spread          its weight-gradient counterpart (ksize 4): dys[n][qi][qj][t] = dy[n][qi - t / 4 + pad][qj - t % 4 + pad][0] (0
 *                          outside), dy [n][hout][wout][ld_dy], dys [n][hin][win][16], both in dtype
 *   vp_pack_inputs         pixrefer.py:373-375, 295-306, 321: inputs [n][hw][6], fg_inputs [n][hw][fg_c] (fg_c 3 or 6) in [0, 1] ->
 *                          gin = (2 in - 1, 0, 0), gfg = (2 fg[0:3] - 1, 0 x 5); train != 0 also din [3n][hw][8] = (in[3:6], fg[3:6], 0, 0) |
 *                          (in[0:3], fg[0:3], 0, 0) | (in[3:6], 0 x 5) and the real half of vin [2n][hw][8] = (fg[3:6], 0 x 5)
 *   vp_composite_fwd_train vp_composite_fwd plus what the training step needs: outputs_fg into channels 3:6 of din's fake group (channels
 *                          0:3 kept, 6:8 zero) and into vin's fake half, and partial[vp_composite_nblocks(n, hw)][2] = per-block
 *                          (sum |2 t - 1 - outputs|, sum |masks - alpha|); din / vin in dtype
 *   vp_composite_bwd       gradient of Gen_loss w.r.t. the pre-tanh generator output: dy4 [n][hw][8] (channels 4:8 zero) from out4,
 *                          outputs, targets, masks, d_din (channels 3:6 used) and d_vin (channels 0:3), both [n][hw][8] in dtype
 *   vp_perceptual          f3 = real half | fake half of conv3_3 (post-relu), `half` elements each: partial[vp_perceptual_nblocks()] =
 *                          per-block sum (fa - fb)^2, df3 = fb > 0 ? -(l1_weight / half) (fa - fb) : 0
 *   vp_loss_final          losses[2] = Gen_loss_L1 = sum comp[.][0] / n_out + sum comp[.][1] / n_out + content, [4] = content =
 *                          sum perc / 2 / n_feat, [3] = losses[1] gan_weight + losses[2] l1_weight; losses[0:2] are read, not written
 * ---------------------------------------------------------------------------------------------- */
enum { VP_BN_PATH_PLANNER = 0, VP_BN_PATH_TWO_PASS = 1, VP_BN_PATH_ONE_LAUNCH = 2 };
size_t vp_bn_groups_workspace_bytes(int groups, int pixels_per_group, int c, int dtype);
int vp_bn_groups_fwd(const void* y, int groups, int pixels_per_group, int c, int dtype, const float* gamma, const float* beta, float eps,
                     float* scale, float* shift, float* mean, float* rstd, void* out_lrelu, void* out_relu, int path, void* workspace,
                     void* stream);
int vp_bn_groups_bwd(const void* y, const void* dz, void* dy, int groups, int pixels_per_group, int c, int dtype, const float* gamma,
                     const float* mean, const float* rstd, float* c1, float* c2, float* dgamma, float* dbeta, float* dbias_zero,
                     int accumulate, int path, void* workspace, void* stream);
int vp_bn_groups_bwd_tail(const void* y, const void* dz, void* dy, int groups, int pixels_per_group, int c, int dtype, const float* gamma,
                          const float* mean, const float* rstd, const double* partial, int nchunk, int raw, float* c1, float* c2,
                          float* dgamma, float* dbeta, float* dbias_zero, int accumulate, void* stream);
int vp_colsum_groups(const void* x, int groups, int pixels_per_group, int c, int creal, int dtype, float* out, int accumulate,
                     void* workspace, void* stream);
int vp_act_apply(const void* y, const float* scale, const float* shift, int groups, int pixels_per_group, int c, int dtype,
                 void* out_lrelu, void* out_relu, void* stream);
int vp_relu_bwd(const void* y, void* d, size_t n, int dtype, void* stream);
int vp_tap_gather(const float* s, const float* bias, float* y, int n, int hin, int win, int ksize, int pad, void* stream);
int vp_tap_spread(const void* dy, int ld_dy, void* dys, int n, int hin, int win, int pad, int dtype, void* stream);
int vp_pack_inputs(const float* inputs, const float* fg_inputs, int fg_c, void* gin, void* gfg, void* din, void* vin, int n, int hw,
                   int train, int dtype, void* stream);
int vp_composite_nblocks(int n, int hw);
int vp_composite_fwd_train(const float* gen_out4, const float* targets, const float* masks, float* out4, float* outputs, float* outputs_fg,
                           void* din, void* vin, double* partial, int n, int hw, int dtype, void* stream);
int vp_composite_bwd(const float* out4, const float* targets, const float* masks, const float* outputs, const void* d_din, const void* d_vin,
                     void* dy4, int n, int hw, float l1_weight, int dtype, void* stream);
int vp_perceptual_nblocks(size_t half, int dtype);
int vp_perceptual(const void* f3, void* df3, double* partial, size_t half, float l1_weight, int dtype, void* stream);
int vp_loss_final(const double* comp_partial, int n_comp, const double* perc_partial, int n_perc, double n_out, double n_feat,
                  float l1_weight, float gan_weight, float* losses, void* stream);
int vp_dwconv7x3_bn_act(const float* x, const float* w, const float* bias, float* y, int b, int h, int wd, int c, void* stream);
int vp_dwconv7x3_bn_act_t(const void* x, const float* w, const float* bias, void* y, int dtype, int b, int h, int wd, int c, void* stream);
int vp_conv_first_fwd(const float* x, const float* w, const float* bias, float* y, int b, int h, int w_in, int cout, void* stream);
size_t vp_dwproj_workspace_bytes(int ce, int cout);
int vp_dwproj_fwd(const float* ex, const float* w_dw, const float* b_dw, const float* w_proj, const float* b_proj, float* y, int add, int b, int h,
                  int w, int ce, int cout, void* workspace, void* stream);
int vp_maxpool_hw(const float* x, float* y, int b, int h, int w, int c, int kh, int kw, int sh, int sw, void* stream);
int vp_gru_seq(const float* xg, const float* xc, const float* whg, const float* whc, const int* seq_len, float* out, int b, int t,
               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rasteriser ("next" row): replaces mesh_core_cython.render_colors_core ->
 * _render_colors_core(image, face_mask, vertices, triangles, colors, depth_buffer, ntri, h, w, c)
 * (utils/cython/mesh_core.h:63, mesh_core.cpp:169-231; caller infer_bfmvid.py:100-108).  Same argument order and
 * in-place convention (image / face_mask / depth_buffer are read-modify-write), plus nver, a batch of frames that share
 * `triangles` (vertices [batch,nver,3], colors [batch,nver,c], outputs [batch,h,w,...]), a workspace and a stream.
 * Bit-exact with the reference: deepest mean-depth triangle wins, ties go to the lowest index, colour (int)(c0+c1+c2)/3.
 * ---------------------------------------------------------------------------------------------- */
size_t vp_render_colors_workspace_bytes(int batch, int h, int w);
int vp_render_colors(unsigned char* image, unsigned char* face_mask, const float* vertices, const int* triangles,
                     const float* colors, float* depth_buffer, int ntri, int nver, int h, int w, int c, int batch,
                     void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The rest of mesh_core_cython (utils/cython/mesh_core_cython.pyx:40-99): the dense correspondence of a frame - which triangle
 * each pixel sees, with which barycentric weights, at which interpolated depth - bit-exact with mesh_core.cpp, batched over frames
 * that share `triangles` like vp_render_colors (vertices [batch,nver,3], buffers [batch,h,w,...]).  All pointers are device pointers,
 * the calls only enqueue, ntri == 0 is legal, h * w < 2^31.
 *
 * Visibility (both rasterisers): a pixel of a triangle's clamped bounding box is a candidate when it lies inside the triangle
 * (isPointInTri, mesh_core.cpp:23-50) or in the two-pixel border ring x < 2, x > w-3, y < 2, y > h-3 (:148, :292: no inside test
 * there, so the weights may leave [0, 1] and the depth is extrapolated).  Its depth is p_depth = w0*d0 + w1*d1 + w2*d2 with
 * get_point_weight's w0 = 1 - u - v, w1 = v, w2 = u (:53-82), in float32, left to right.  The reference overwrites on a strictly
 * greater depth in index order, so the survivor is the greatest p_depth and, among equal ones, the lowest index; a NaN p_depth never
 * wins, and a pixel that no candidate beats keeps every buffer as given (a second call over the same buffers changes nothing).
 * A triangle with a vertex index outside 0 .. nver-1 is skipped (the reference reads out of bounds).
 *
 * vp_rasterize_triangles: _rasterize_triangles_core(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, nver, ntri,
 *   h, w) (mesh_core.h:57, mesh_core.cpp:108-166).  depth_buffer f32 [batch,h,w], triangle_buffer i32 [batch,h,w], barycentric_weight
 *   f32 [batch,h,w,3] are read-modify-write: winning pixels get the winner's depth, index and weights.
 * vp_render_texture: _render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth_buffer, nver, tex_nver,
 *   ntri, h, w, c, tex_h, tex_w, tex_c, mapping_type) (mesh_core.h:70, mesh_core.cpp:234-333).  image f32 [batch,h,w,c] and depth_buffer
 *   are read-modify-write; texture f32 [tex_h,tex_w,tex_c], tex_coords f32 [tex_rows,3] and tex_triangles i32 [ntri,3] are shared by the
 *   frames.  The indexing is the reference's as written (:270-272): x of corner k is tex_coords[3*tex_triangles[3i+k]], y is
 *   tex_coords[3*triangles[3i+k] + 1]; tex_p = tex_p0*w0 + tex_p1*w1 + tex_p2*w2, clamped to the texture; mapping_type 0 reads the
 *   nearest texel through round() (half away from zero), any other value the four-term bilinear sum in the written order (:322).
 *   Refused: c > tex_c, tex_rows < max(nver, tex_nver).  A triangle with a tex_triangles index outside 0 .. tex_nver-1 is skipped.
 * vp_raster_interpolate: no compiled form in the reference (its callers do this in numpy): out[f,y,x,:] = w0*a[i0] + w1*a[i1] + w2*a[i2]
 *   in float32, left to right, for the pixel's triangle (i0,i1,i2) and weights; attributes f32 [batch,nver,k], out f32 [batch,h,w,k].
 *   Pixels whose triangle_buffer entry is negative (or not below ntri) are left as given.
 * vp_vertex_normals: _get_normal_core(normal, tri_normal, triangles, ntri) (mesh_core.h:53, mesh_core.cpp:85-105): normal [batch,nver,3]
 *   += tri_normal [batch,ntri,3] of the incident triangles, added in ascending triangle order and within a triangle in corner order (a
 *   repeated index adds twice), onto the values given: the bits of the serial loop.  The order comes from an adjacency (vertex ->
 *   sorted list of 3*triangle + corner) that depends on `triangles` alone: vp_vertex_adjacency_build fills `adjacency`
 *   (vp_vertex_adjacency_bytes(nver, ntri) bytes, 0 for bad sizes) once, vp_vertex_normals takes it with the same nver and ntri.
 *   Corners with an index outside 0 .. nver-1 are left out of it.
 * vp_raster_vertex_visibility: no counterpart in the reference.  Is a vertex of the mesh that was rasterised in front of the surface the
 *   depth buffer holds?  vertices f32 [batch,nver,3] as the rasteriser was given them, depth_buffer f32 [batch,h,w] as
 *   vp_rasterize_triangles left it, visible u8 [batch,nver].  In float32, for a vertex (x, y, z): 1 when x, y or z is a NaN or x < 0,
 *   x > w-1, y < 0, y > h-1 (the buffer says nothing about it); otherwise x0 = min((int)floorf(x), w-2), y0 likewise, m = the minimum
 *   (fminf: a NaN depth is ignored) of the depths at (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1), and visible = (z + tol >= m).  The four
 *   pixel centres surround the vertex; on its own, locally planar, surface at least one of them is no nearer than the vertex, so no
 *   slope-dependent tolerance is needed (only a concave dip deeper than tol can fail).  An occluder that covers all four centres hides
 *   the vertex; a vertex on an occlusion edge stays visible; an empty pixel (the caller's clear value) makes it visible.
 *   Refused: h or w < 2, nver or batch < 1, tol negative or not finite.
 * ---------------------------------------------------------------------------------------------- */
size_t vp_rasterize_triangles_workspace_bytes(int batch, int h, int w);
int vp_rasterize_triangles(const float* vertices, const int* triangles, float* depth_buffer, int* triangle_buffer, float* barycentric_weight,
                           int nver, int ntri, int h, int w, int batch, void* workspace, void* stream);
size_t vp_render_texture_workspace_bytes(int batch, int h, int w);
int vp_render_texture(float* image, const float* vertices, const int* triangles, const float* texture, const float* tex_coords,
                      const int* tex_triangles, float* depth_buffer, int nver, int tex_nver, int tex_rows, int ntri, int h, int w, int c, int tex_h,
                      int tex_w, int tex_c, int mapping_type, int batch, void* workspace, void* stream);
int vp_raster_interpolate(float* out, const int* triangle_buffer, const float* barycentric_weight, const int* triangles, const float* attributes,
                          int nver, int ntri, int k, int h, int w, int batch, void* stream);
size_t vp_vertex_adjacency_bytes(int nver, int ntri);
int vp_vertex_adjacency_build(const int* triangles, int nver, int ntri, void* adjacency, size_t adjacency_bytes, void* stream);
int vp_vertex_normals(float* normal, const float* tri_normal, const void* adjacency, int nver, int ntri, int batch, void* stream);
int vp_raster_vertex_visibility(const float* vertices, const float* depth_buffer, unsigned char* visible, int nver, int h, int w, int batch, float tol,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * BFM reconstruction for a clip ("next" row): replaces the per-frame numpy of
 * utils/reconstruct_mesh.py Reconstruction_rotation(coeff, facemodel, angles) (:198-223) and the float32 / integer packing
 * of infer_bfmvid.py:92-99.  All pointers are device pointers.  The model is the reference's `BFM` object
 * (utils/bfm_load_data.py:9-21) promoted to float64 with 0-based indices: tri [ntri,3]; point_buf [nver,8] with `ntri`
 * marking "no face" (the reference's appended zero normal, reconstruct_mesh.py:47-49).  `center` = column means of
 * meanshape (:27), `sh` = {a0c0, a1c1, a2c2, a2c2/2/sqrt(3), a2c2/2} of Illumination_layer (:138-155), both evaluated
 * by the host in double; focal / image_center are Projection_layer's 1015 / 112 (:100-101).
 * coeff [frames,257] float32; rotation [frames,9] = Compute_rotation_matrix(angles) (:68-93) row-major, float64.
 * Outputs: vertices [frames,nver,3] = (x, 224-y, z_buffer) float32 and colors [frames,nver,3] = float(int(clip(c,0,255))),
 * i.e. exactly the arrays infer_bfmvid.py:101-103 passes to render_colors_core; the float64 intermediates the reference
 * returns (face_shape, face_texture, face_color, face_projection [.,.,2], z_buffer) are written when non-NULL.
 * shared_texture != 0: the texture coefficients are constant over the clip, computed once from frame 0
 * (face_texture then holds 1 frame).
 * ---------------------------------------------------------------------------------------------- */
typedef struct vp_bfm_model {
  int nver, ntri;
  const double* meanshape; /* [3*nver] */
  const double* idBase;    /* [80,3*nver]  K-MAJOR: the reference's [3*nver,80] transposed once at model load */
  const double* exBase;    /* [64,3*nver] */
  const double* meantex;   /* [3*nver] */
  const double* texBase;   /* [80,3*nver] */
  const int* tri;          /* [ntri,3] */
  const int* point_buf;    /* [nver,8] */
  double center[3];
  double focal, image_center;
  double sh[5];
} vp_bfm_model;
size_t vp_bfm_reconstruct_workspace_bytes(int nver, int ntri, int frames);
int vp_bfm_reconstruct(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, int shared_texture,
                       double* face_shape, double* face_texture, double* face_color, double* face_projection, double* z_buffer,
                       float* vertices, float* colors, void* workspace, size_t workspace_bytes, void* stream);
/* The same for rows of several identities in one call (stream groups: frames of many talkers in one render launch chain).  The
 * texture - vp_bfm_reconstruct(shared_texture = 1) computes it once, from row 0 - is computed once per identity present: texture t
 * (0 .. textures-1) from the coefficients of row tex_src[t], and row r is lit with texture tex_row[r].  tex_src [textures] and
 * tex_row [frames] are DEVICE int arrays (the caller sends them with its other per-push tables); entries out of range leave the
 * row unwritten.  Per-row arithmetic is that of vp_bfm_reconstruct: the rows of one identity equal, bit for bit, what
 * vp_bfm_reconstruct(shared_texture = 1) returns for that identity's frames alone.  Same workspace query; never waits. */
int vp_bfm_reconstruct_rows(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, const int* tex_src, int textures,
                            const int* tex_row, float* vertices, float* colors, void* workspace, size_t workspace_bytes, void* stream);

/* Reconstruction(coeff, facemodel) (utils/reconstruct_mesh.py:172-194), the form plot_bfm_coeff_seq (utils/bfm_visual.py:97) and
 * voicepuppet/bfmnet/infer_bfmnet.py:209 call: the pose is the coefficients' own, rotation [frames,9] = Compute_rotation_matrix(coeff[:, 224:227])
 * (evaluated by the host in double, as above).  The normals are rotated by it, the projection is shape . R + t (ONE rotation, inside
 * Projection_layer), and face_shape is returned UNROTATED; lighting and colour packing are those of vp_bfm_reconstruct.  No choice of
 * angles turns vp_bfm_reconstruct into this.  Same model, same workspace query, same optional float64 outputs.
 *   view 0 (montage, bfm_visual.py:100-112):  vertices = float32(x, 224 - y, z_buffer); scale is ignored
 *   view 1 (mesh video, infer_bfmnet.py:212-216): vertices = float32((112 - sx*112)*scale, (112 - sy*112)*scale, sz*scale) from the
 *          unrotated face_shape, evaluated in double in that order; the reference's scale is 3 (a 672 x 672 image); 0 < scale <= 1024 */
int vp_bfm_reconstruct_view(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, int shared_texture, int view, double scale,
                            double* face_shape, double* face_texture, double* face_color, double* face_projection, double* z_buffer,
                            float* vertices, float* colors, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Visual evaluation of BFMNet: the mesh montage of utils/bfm_visual.py plot_bfm_coeff_seq (:88-154) and a number to go with it.
 * vp_sheet_tile_u8: tile i of tiles [n,h,w,3] uint8 (vp_render_colors' images) goes to cell first_cell + i of sheet
 * [sheet_rows*h, sheet_cols*w, 3] uint8: cell c is row c / sheet_cols, column c % sheet_cols (:127-128).  swap_rb != 0 exchanges the
 * first and third channel on the way (:125).  Cells that are not written keep their contents: the caller zeroes the sheet.  A cell
 * outside the sheet is refused with VP_ERR_ARG before anything is enqueued.
 * vp_landmark_distance: for frame f of two projected sequences proj_a, proj_b [frames,nver,2] float64 (face_projection of view 0: pixels
 * of the 224 image) and keypoints [68] int32 (0-based vertex indices, facemodel.keypoints), out[f] = { mean over the 68 landmarks of the
 * Euclidean distance, the same over landmarks 48..67 (the mouth) }.  One wavefront per frame and a fixed summation order: a frame's two
 * numbers are the same bits alone and in any batch.  A keypoint outside 0 .. nver-1 is not read; the frame's numbers are NaN.
 * ---------------------------------------------------------------------------------------------- */
int vp_sheet_tile_u8(const unsigned char* tiles, int n, int h, int w, unsigned char* sheet, int sheet_rows, int sheet_cols, int first_cell,
                     int swap_rb, void* stream);
int vp_landmark_distance(const double* proj_a, const double* proj_b, const int* keypoints, int frames, int nver, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fit of BFM coefficients to 68 landmarks: the inverse of `Reconstruction` (utils/reconstruct_mesh.py:172-194) for its landmarks_2d.
 * Replaces the coefficient regression of FaceReconModel.pb (voicepuppet/pixrefer/infer_bfmvid.py:47-74, datasets/make_data_from_GRID.py:193-214)
 * for identity 0:80, expression 80:144, angles 224:227 and translation 254:257; texture 144:224 and lighting 227:254 are NOT fitted by these two calls and keep
 * the template's values (vp_bfmfit_appearance, below, fits them to a photo).  Unknowns p[150] = [alpha | beta | angles | t]; cost E = sum_k w_k |pi_k(p) - l_k|^2 + lam_id |alpha|^2 + lam_ex |beta|^2,
 * pi = the forward model above (re-centred shape, ONE rotation (Rz Ry Rx)^T, + t, z -> 10 - z, focal / image_center of the model, y -> 224 - y,
 * taken at the keypoints).  Levenberg-Marquardt in float64: A = J^T W J + Lambda, g = J^T W r + Lambda p on the free parameters; status 0 when
 * |g|_inf <= gtol; (A + mu diag A) d = -g by Cholesky; E(p + d) < E(p) accepts and mu <- max(mu / 3, 1e-9), anything else (a non-finite cost
 * included) rejects and mu <- 4 mu; mu > 1e8: status 2; max_iters accepted steps: status 1; non-finite landmarks or start values: status 3 and
 * the start values go back.  mu0 = 1e-3.  Every loop is bounded by these rules.
 * The two costs of that comparison leave out the regularisation of the blocks that are not free (the same number on both sides; it would only
 * set their rounding); the reported E is the whole cost.
 *   keypoints [68]    HOST int array, 0-based vertex indices (facemodel.keypoints); one outside 0 .. nver-1 is refused before any launch
 *   table_ready       0: the keypoint rows of the model are gathered into the workspace first (one more launch); != 0: the caller
 *                     states that an earlier call with this model, these keypoints and this workspace has done that
 *   landmarks         [frames,68,2] float64 (x, y) pixels of the 224 image
 *   weights           NULL (all 1), [68] (weights_per_frame = 0) or [frames,68]; w <= 0 drops the landmark
 *   init              [frames,257] float32: start values and template
 *   params            optional [frames,150] float64: p as float64 on return; with params_in != 0 also the start values (instead of init's)
 *   free_mask         bits 1 identity, 2 expression, 4 angles, 8 translation: 15 full fit, 14 tracking, 12 pose only
 *   coeff             [frames,257] float32 (may be init): the template with the fitted blocks overwritten; other blocks bit-equal to init
 *   report            [frames,4] float64 = { status, accepted iterations, final E, final |g|_inf }
 * One workgroup per frame, fixed summation order: a frame's coeff, params and report are the same bits alone and in any batch.
 * vp_bfmfit_identity_step: one Gauss-Newton step on an alpha shared by all frames (row 0's alpha is taken as the current one), beta and pose of
 * every frame fixed: A = sum_t J_a^T W J_a + T lam_id I, g = sum_t J_a^T W r_t + T lam_id alpha, summed over blocks of 64 consecutive frames
 * and then over the blocks, both in frame order (no atomics); alpha + d goes to columns 0:80 of every row of params (and of coeff, when
 * non-NULL, as float32).  Frames with non-finite landmarks or parameters take no part (T counts the others).  Neither call waits.
 * ---------------------------------------------------------------------------------------------- */
size_t vp_bfmfit_workspace_bytes(int frames);
int vp_bfmfit_fit(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights, int weights_per_frame,
                  const float* init, double* params, int params_in, int frames, double lam_id, double lam_ex, double gtol, int max_iters, int free_mask,
                  float* coeff, double* report, void* workspace, size_t workspace_bytes, void* stream);
int vp_bfmfit_identity_step(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights,
                            int weights_per_frame, double* params, float* coeff, int frames, double lam_id, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Joint fit of a clip to its landmarks: ONE identity for the clip, expression and pose per frame, optionally coupled in time.  The same
 * inverse of `Reconstruction` (utils/reconstruct_mesh.py:172-194) as vp_bfmfit_fit and the same replacement of FaceReconModel.pb
 * (voicepuppet/pixrefer/infer_bfmvid.py:47-74, datasets/make_data_from_GRID.py:193-214), for the rows of a clip's bfmcoeff.txt: what
 * BFMNet's loss (voicepuppet/bfmnet/bfmnet.py add_cost_function) differences in time.  A clip has frames t = 1 .. T; unknowns alpha (80) and
 * q_t = [beta_t (64) | angles (3) | t (3)], 80 + 70 T numbers, a frame's parameters laid out as vp_bfmfit_fit's p[150]:
 *   E = sum_t ( sum_k w_tk |pi_k(alpha, q_t) - l_tk|^2 + lam_id |alpha|^2 + lam_ex |beta_t|^2 )                  (T lam_id |alpha|^2 in all)
 *     + sum_{t<T} ( s_ex |beta_t+1 - beta_t|^2 + s_ang |ang_t+1 - ang_t|^2 + s_t |t_t+1 - t_t|^2 ),   lam_smooth = (s_ex, s_ang, s_t)
 * With lam_smooth = (0, 0, 0) this is the sum of vp_bfmfit_fit's cost over the frames for a shared alpha.  Useful values of lam_smooth are
 * UNTUNED on real landmark files.
 * Levenberg-Marquardt in float64 on the whole clip, the rule of vp_bfmfit_fit: A = J^T W J + Lambda + the coupling's Hessian, g likewise;
 * (A + mu diag A) d = -g by Cholesky; E falls: accept, mu <- max(mu / 3, 1e-9); anything else (a non-finite cost included) rejects,
 * mu <- 4 mu; mu > 1e8: status 2; mu0 = 1e-3; a factorisation that fails raises mu the same way without an evaluation; status 0 when
 * |g|_inf <= gtol over all 80 + 70 T unknowns; status 1 when max_trials trial points have been evaluated; status 3 for non-finite landmarks
 * or start values, and the start values go back.  "E falls" is sum_t (E_t(trial) - E_t(current)) + (coupling(trial) - coupling(current)) < 0,
 * added in frame order: not a difference of two clip totals, so the float64 floor of the test stays at one frame's magnitude.
 * A is block arrowhead: 70x70 frame blocks on a chain whose off-diagonal blocks are -diag(s), bordered by the 70x80 alpha coupling, corner
 * 80x80.  A fit is a fixed chain of launches (init, frames, (clip, frames) x max_trials, clip), nothing is read back: `frames` (one
 * workgroup per frame) evaluates a frame's 150x150 system at the trial point, `clip` (one workgroup per clip) applies the rule, eliminates
 * the chain by a block Cholesky sweep forward over t (per-frame factors kept in the workspace), solves the corner's Schur complement,
 * substitutes back and writes the next trial point.  Both leave a clip with a status alone.  Fixed summation order, no atomics: a clip's
 * coeff, params and report are the same bits alone and in any batch.  The sweep is serial in t.
 *   keypoints, table_ready, landmarks [F,68,2], weights, weights_per_frame    as for vp_bfmfit_fit; the table lives in THIS call's workspace
 *   clip_offsets      HOST int32 [clips+1]: clip c is frames clip_offsets[c] .. clip_offsets[c+1]-1; clip_offsets[0] = 0, F = clip_offsets[clips]
 *   coeff_in          [F,257] float32: the template (texture, lighting)
 *   params            [F,150] float64, in and out: the start values (alpha is taken from the clip's FIRST row, as vp_bfmfit_identity_step
 *                     takes it) and the solution
 *   lam_smooth        HOST double [3]
 *   max_trials        0: only E and |g|_inf at the start values are reported (status 0 or 1)
 *   coeff             [F,257] float32 (may be coeff_in): the template with the fitted blocks overwritten
 *   report            [clips,4] float64 = { status, accepted steps, final E, final |g|_inf }
 * Refused on the host before anything is enqueued: a null pointer, clips < 1, a keypoint outside the model, clip_offsets[0] != 0, offsets
 * that do not increase (a clip of 0 frames), a negative or non-finite lam or lam_smooth, gtol < 0, max_trials outside 0 .. 100000, a short
 * workspace.  The call does not wait.
 * ---------------------------------------------------------------------------------------------- */
size_t vp_bfmfit_clip_workspace_bytes(int total_frames, int clips);
int vp_bfmfit_clip(const vp_bfm_model* m, const int* keypoints, int table_ready, const double* landmarks, const double* weights, int weights_per_frame,
                   const int* clip_offsets, int clips, const float* coeff_in, double* params, double lam_id, double lam_ex, const double* lam_smooth,
                   double gtol, int max_trials, float* coeff, double* report, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Photometric fit of texture (coefficients 144:224) and lighting (227:254) to a photo's pixels, the geometry fixed at what vp_bfmfit_fit
 * returned: the inverse of face_color = Illumination_layer(Texture_formation(tex_coeff), face_norm . rotation, gamma)
 * (utils/reconstruct_mesh.py:58-62, :129-168, as Reconstruction :172-194 calls them; render_face rasterises that colour,
 * voicepuppet/pixrefer/infer_bfmvid.py:91-108).  Replaces, for those 107 coefficients, FaceReconModel.pb (infer_bfmvid.py:47-74).
 * For frame f, vertex v, channel c (RGB, :57), unknowns p[107] = [delta(80) | gamma(27)]:
 *   T_vc = meantex_vc + sum_j texBase[3v+c, j] delta_j                                   (:59)
 *   L_vc = sum_k Y_vk (gamma_ck + init_k),  init = (0.8, 0, ..., 0), gamma viewed as [3,9]  (:133-135, :159-161)
 *   Y_v  = the nine SH terms (:137-155) of the ROTATED normal n_v . R (:182)
 *   r_vc = T_vc L_vc - I_vc,  I_v the photo sampled at the vertex's projection;  colours in the reference's 0 .. 255 units
 *   E    = (1/W) sum_v w_v sum_c r_vc^2 + lam_tex |delta|^2 + lam_gamma |gamma|^2,   W = 3 sum_v w_v
 * (1/W keeps lam meaningful at any vertex count.)  lam_tex = lam_gamma = 1 are the callers' defaults and are UNTUNED on real photos.
 *
 * vp_bfmfit_observe (inverts :179-186, the geometry half of Reconstruction): face_shape, the one-ring normals, n . R and face_projection
 * exactly as vp_bfm_reconstruct_view computes them (the same device code), then
 *   sh [frames,nver,9]       Y_v
 *   observed [frames,nver,3] the photo sampled bilinearly, in float64, at (a x + bx, a y + by), (x, y) = face_projection, integer
 *                            coordinates = pixel centres; 0 where the position is outside
 *   weight [frames,nver]     vertex_weights_v max(0, (n_v . R)_z) inside: the camera sits at z = +10 (:103), normals facing it have positive z;
 *                            inside = 1 iff 0 <= px <= W-1 and 0 <= py <= H-1
 * coeff [frames,257] float32; rotation [frames,9] float64 = Compute_rotation_matrix(coeff[:, 224:227]) from the host, as for
 * vp_bfm_reconstruct_view; frames <= 65535; photo [photo_frames,H,W,3] uint8 RGB, photo_frames 1 (shared) or frames, H, W >= 2; affine [frames,3] float64
 * (a, bx, by): 224-image pixels -> photo pixels; vertex_weights NULL (ones) or [nver] float64 (a skin mask).  All device pointers.
 * This call has no self-occlusion test (the facing weight is smooth, so no threshold can flip) and reads ONE bilinear tap whatever a is;
 * vp_bfmfit_observe_ex adds both as options.
 *
 * vp_bfmfit_observe_ex: vp_bfmfit_observe's arguments, refusals and, with visibility = prefilter = 0, its bits (the geometry, sh, the
 * inside test and the facing weight are the same device code), then `o` and `visible` (NULL or u8 [frames,nver]):
 *   visibility = 1   per frame, float32 raster vertices (ss x, ss y, z_buffer): (x, y) = face_projection, z_buffer what view 0 of
 *                    vp_bfm_reconstruct_view packs (greater = nearer), ss = raster_scale, the products in float64 and then rounded;
 *                    depth cleared to -99999 and triangle ids to -1; vp_rasterize_triangles into a (224 ss)^2 buffer;
 *                    vp_raster_vertex_visibility with tol = depth_tol (model units, decimetres); weight is multiplied by the 0 / 1 result,
 *                    which also goes to `visible`.  Frames pass through the raster buffers in chunks of at most 8, so the workspace is
 *                    frames x (a per-frame size) + a constant.  With visibility = 0, `visible` is not written.
 *   prefilter = 1    a frame with a > 1 reads k x k bilinear taps per vertex, k = min(ceil(a), 16), at (px + ((i + 0.5) / k - 0.5) a,
 *                    py + ((j + 0.5) / k - 0.5) a), each coordinate clamped to [0, W-1] x [0, H-1]; observed is their mean, in float64;
 *                    inside is still the centre's.  Order of the sum: tap t = i + k j (i along x) belongs to lane t % 64 of a wave; a lane
 *                    adds its taps in ascending t; the 64 lane sums are combined by an xor butterfly, strides 32, 16, 8, 4, 2, 1; the total
 *                    is divided by k k.  It depends on k alone: a frame's numbers are the same bits in any batch.  A frame with a <= 1 takes
 *                    vp_bfmfit_observe's single tap, bit for bit.
 * Refused on the host before anything is enqueued: a struct_bytes other than vp_bfmfit_observe_opts_size(), visibility / prefilter not
 * 0 or 1, raster_scale not 1, 2 or 4, a negative or non-finite depth_tol, everything vp_bfmfit_observe refuses, a short workspace.
 * depth_tol = 0.01 (1 mm) is the Python callers' default and is UNTUNED on real photos.
 *
 * vp_bfmfit_appearance (inverts :58-62 and :129-168): Levenberg-Marquardt in float64 on p, the rule of vp_bfmfit_fit with
 *   A = J^T W J / W + Lambda, g = J^T W r / W + Lambda p;  d r_vc / d delta_j = L_vc texBase[3v+c, j];  d r_vc / d gamma_ck = Y_vk T_vc
 *   (A + mu diag A) d = -g by Cholesky;  E(p + d) < E(p) accepts and mu <- max(mu / 3, 1e-9); anything else rejects and mu <- 4 mu;
 *   mu > 1e8: status 2;  mu0 = 1e-3;  a factorisation that fails raises mu the same way without an evaluation
 *   status 0 when |g|_inf <= gtol E, or E = 0: a RELATIVE test, because the float64 floor of the accept test scales with E
 * A fit is a fixed chain of max_trials rounds (accumulate, step) and nothing is read back.  The accumulate stage evaluates (A, g, E) at
 * the trial point: blocks own vertex slabs (the partition a function of nver alone) and write partial systems per (frame, slab); a second
 * launch adds them in slab order, no atomics.  The step kernel (one workgroup per frame) applies the rule, keeps the system of the last accepted point, solves for the next
 * trial point and sets the status; both leave a frame with a status alone.  A frame's coeff, params and report are therefore the same
 * bits alone and in any batch.  Status 1: max_trials evaluations were used up; status 3: a non-finite sh / weight / observed / start
 * value or sum_v w_v = 0, and the start values go back.
 *   sh, weight, observed   vp_bfmfit_observe's outputs (weight <= 0 drops a vertex)
 *   coeff_in               [frames,257] float32: template, and start values unless params_in
 *   params                 optional [frames,107] float64: p on return; with params_in != 0 also the start values
 *   stages                 3 in every use but timing.  1 / 2 enqueue only the accumulate stage / only the step launches of the chain, so that
 *                          the two can be timed apart: with 1, coeff, report and params are NOT written (undefined on return); with 2 they
 *                          come from whatever partial sums the workspace holds
 *   coeff                  [frames,257] float32 (may be coeff_in): columns 144:224 and 227:254 fitted, every other column copied
 *   report                 [frames,4] float64 = { status, accepted steps, E, |g|_inf } at the returned point
 * Neither call waits.
 * ---------------------------------------------------------------------------------------------- */
size_t vp_bfmfit_observe_workspace_bytes(int nver, int ntri, int frames);
int vp_bfmfit_observe(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, const unsigned char* photo, int photo_frames,
                      int height, int width, const double* affine, const double* vertex_weights, double* sh, double* weight, double* observed,
                      void* workspace, size_t workspace_bytes, void* stream);
typedef struct vp_bfmfit_observe_opts {
  uint32_t struct_bytes;   /* sizeof(vp_bfmfit_observe_opts) of the caller's build: must equal vp_bfmfit_observe_opts_size() */
  int32_t visibility;      /* 0 | 1 */
  int32_t raster_scale;    /* ss: 1, 2 or 4; the depth raster is (224*ss)^2 */
  int32_t prefilter;       /* 0 | 1 */
  float depth_tol;         /* model units (decimetres), >= 0 */
} vp_bfmfit_observe_opts;
size_t vp_bfmfit_observe_opts_size(void);
size_t vp_bfmfit_observe_ex_workspace_bytes(int nver, int ntri, int frames, const vp_bfmfit_observe_opts* o);
int vp_bfmfit_observe_ex(const vp_bfm_model* m, const float* coeff, const double* rotation, int frames, const unsigned char* photo, int photo_frames,
                         int height, int width, const double* affine, const double* vertex_weights, double* sh, double* weight, double* observed,
                         void* workspace, size_t workspace_bytes, void* stream, const vp_bfmfit_observe_opts* o, unsigned char* visible);
size_t vp_bfmfit_appearance_workspace_bytes(int nver, int frames);
int vp_bfmfit_appearance(const vp_bfm_model* m, const double* sh, const double* weight, const double* observed, const float* coeff_in, double* params,
                         int params_in, int frames, double lam_tex, double lam_gamma, double gtol, int max_trials, int stages, float* coeff,
                         double* report, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BFMNet TRAINING step (voicepuppet/bfmnet/bfmnet.py:215-323, tinynet.py:7-212): the non-GEMM kernels, float32 NHWC,
 * any channel count that is a multiple of 4.  voicepuppet_amd/bfmnet/train_engine.py chains them with plain GEMMs (rocBLAS).
 *   vp_bn_train_fwd / _bwd   tf.contrib.layers.batch_norm(is_training=True, scale=False, eps 1e-3): batch statistics + the affine that
 *                            normalises (y = x * scale + shift), and its backward (dx, dbeta)
 *   vp_bn_act_train_bwd      the same with the backward of the relu / relu6 that follows folded in (no dz tensor is materialised)
 *   vp_affine_act_fwd        y = act(scale[c] * x + shift[c]) * mask (affine and mask optional: relu / relu6 / leaky-relu, dropout)
 *   vp_act_bwd               dx = dy * mask * act'(y)
 *   vp_dwconv7x3_raw         depthwise [7,3] SAME without bias / activation (forward; backward-data with reversed taps);
 *   vp_dwconv7x3_wgrad       its weight gradient [21][c]
 *   vp_maxpool_hw_bwd        backward of vp_maxpool_hw (first maximum of a window, as TF's MaxPoolGrad)
 *   vp_stem_im2col           the 9x5 stride-(1,2) stem as a [pixels, 48] matrix (GEMM operand for forward and weight gradient)
 *   vp_gru_train_fwd / _bwd  GRUCell recurrence with saved gates, and backward through time to the gate / candidate pre-activations.
 *                            whg [256][512] / whc [256][256]: the recurrent halves of the two kernels (row = h unit).  _bwd takes them
 *                            TRANSPOSED (whg_t [512][256], whc_t [256][256]): its products with the kernels' rows then read coalesced columns
 *   vp_bfm_vertex_loss       add_cost_function on D = face_shape(true) - face_shape(pred): loss partials (f64) and dLoss/dD
 *   vp_sumsq                 sum of squares partials (f64): global-norm clipping
 *   vp_l2_regulariser        tf.losses.get_regularization_loss() over the flat arena: gradient contribution + value partials
 *   vp_adam_tf_clipped       tf.clip_by_global_norm + tf.train.AdamOptimizer (bfmnet.py:313-318) with the step scalars on the device
 *   vp_moving_update         the moving-average updates of every batch_norm in one pass (decay 0.999, tinynet.py:20-27)
 * ---------------------------------------------------------------------------------------------- */
size_t vp_bn_train_workspace_bytes(size_t pixels, int c);
int vp_bn_train_fwd(const float* x, size_t pixels, int c, const float* beta, float eps, float* mean, float* var, float* rstd, float* scale,
                    float* shift, void* workspace, void* stream);
int vp_bn_train_bwd(const float* x, const float* dz, size_t pixels, int c, const float* mean, const float* rstd, float* dx, float* dbeta,
                    void* workspace, void* stream);
int vp_bn_act_train_bwd(const float* x, const float* da, size_t pixels, int c, const float* mean, const float* rstd, const float* shift, int act,
                        float* dx, float* dbeta, void* workspace, void* stream);
int vp_affine_act_fwd(const float* x, const float* scale, const float* shift, const float* mask, size_t pixels, int c, int act, float* y, void* stream);
/* the same pass + the residual branch: y = act(scale * x + shift) * mask + add */
int vp_affine_act_add_fwd(const float* x, const float* scale, const float* shift, const float* mask, const float* add, size_t pixels, int c, int act,
                          float* y, void* stream);
int vp_act_bwd(const float* dy, const float* ya, const float* mask, size_t n, int act, float* dx, void* stream);
int vp_dwconv7x3_raw(const float* x, const float* w, float* y, int b, int h, int wd, int c, void* stream);
/* backward-data of vp_dwconv7x3_raw: dy convolved with the taps of w reversed (no flipped copy of w is needed) */
int vp_dwconv7x3_bwd_data(const float* dy, const float* w, float* dx, int b, int h, int wd, int c, void* stream);
size_t vp_dwconv7x3_wgrad_workspace_bytes(int b, int h, int wd, int c);
int vp_dwconv7x3_wgrad(const float* x, const float* dy, float* dw, int b, int h, int wd, int c, void* workspace, void* stream);
int vp_maxpool_hw_bwd(const float* x, const float* dy, float* dx, int b, int h, int w, int c, int kh, int kw, int sh, int sw, void* stream);
int vp_stem_im2col(const float* x, float* col, int b, int h, int w, void* stream);
int vp_gru_train_fwd(const float* xg, const float* xc, const float* whg, const float* whc, const int* seq_len, float* out, float* r, float* u, float* c,
                     float* hprev, int b, int t, void* stream);
/* glue of the training step (bias gradients = column sums over the B*T rows, the recurrent halves of the GRUCell kernels split and
 * transposed in one launch, element-wise products of the dropout masks / gate products, the ear padding of bfmnet.py:117,210) */
int vp_colsum_f32(const float* x, int rows, int cols, float* out, void* stream);
int vp_gru_split_recurrent(const float* gates_kernel, const float* cand_kernel, float* whg, float* whc, float* whg_t, float* whc_t, void* stream);
int vp_mul_f32(const float* a, const float* b, float* out, size_t n, void* stream);
int vp_add_ears_f32(float* out, const float* ears, int rows, void* stream);
int vp_gru_train_bwd(const float* dout, const float* whg_t, const float* whc_t, const int* seq_len, const float* r, const float* u, const float* c,
                     const float* hprev, float* dag, float* dac, int b, int t, void* stream);
int vp_vertex_loss_partials(int b, int j);
int vp_bfm_vertex_loss(const float* d, const float* vmask, const int* seq_len, int b, int t, int j, float* gd, double* partial, void* stream);
int vp_sumsq_partials(size_t n);
int vp_sumsq(const float* x, size_t n, double* partial, void* stream);
int vp_l2_regulariser(const float* params, const float* mask, float* grads, size_t n, float scale, double* partial, void* stream);
/* The step's scalars on the device (no framework reduction / sqrt / stack on the path): out[0] = (add ? add[0] : 0) + scale * sum(partial[0..n));
 * out3 = [loss_data + half_l2 * reg, loss_data, sqrt(sumsq)]; grads *= clip / max(sqrt(sumsq), clip).  All pointers are device memory. */
int vp_sum_f64(const double* partial, int n, double scale, const double* add, double* out, void* stream);
int vp_bfm_step_report(const double* loss_data, const double* reg, double half_l2, const double* sumsq, double* out3, void* stream);
int vp_clip_scale_f32(float* grads, size_t n, const double* sumsq, float clip, void* stream);
int vp_adam_tf_clipped(float* params, float* grads, float* m, float* v, size_t n, const float* lr_t, const double* sumsq, float clip, float beta1,
                       float beta2, float eps, void* stream);
int vp_moving_update(float* moving, const float* batch, const float* factor, size_t n, float decay, void* stream);

/* ---- plain float32 matrix products on the repo's own MFMA kernels (the BFMNet training step is made of them: bfmnet.py:215-323) ----
 * Row-major, leading dimensions in floats.  vp_mm_fwd_f32: y[P,N] = x[P,K] . w[K,N] (+ bias[N]); w_transposed: w is stored [N,K].
 * vp_mm_bwd_data_f32: dx[P,K] (+)= dy[P,N] . w[K,N]^T.  vp_mm_bwd_weight_f32: dw[k_real,N] = (x[P,K]^T . dy[P,N])[:k_real].
 * The contraction dimension of the first two (K resp. N) is walked in chunks of 16 floats: K % 16 == 0, and dy carries
 * lddy >= round_up(N, 16) columns with zeros beyond N.  workspace: vp_mm_workspace_bytes(P, K, N) device bytes (the packed
 * copy of w, split-K slabs) whose FIRST 256 BYTES ARE ZERO on entry; the calls never write them.  float32 products and
 * accumulation (v_mfma_f32_16x16x4_f32). */
size_t vp_mm_workspace_bytes(int P, int K, int N);
int vp_mm_fwd_f32(const float* x, int ldx, const float* w, int ldw, int w_transposed, const float* bias, float* y, int ldy,
                  int P, int K, int N, void* workspace, void* stream);
int vp_mm_bwd_data_f32(const float* dy, int lddy, const float* w, int ldw, int w_transposed, float* dx, int lddx, int accumulate,
                       int P, int K, int N, void* workspace, void* stream);
int vp_mm_bwd_weight_f32(const float* x, int ldx, const float* dy, int lddy, float* dw, int P, int K, int k_real, int N,
                         void* workspace, void* stream);
/* The same two weight-consuming products on weights packed AHEAD of time (a training step re-packs every matrix once, in one
 * launch, instead of once per product).  dir: 0 = the layout of vp_mm_fwd_f32, 1 = of vp_mm_bwd_data_f32; the layout follows from
 * (P, K, N, dir) alone.  vp_mm_pack_desc fills one host descriptor (vp_mm_pack_desc_bytes() bytes) of a matrix at master + w_off
 * floats whose packed block goes to packed + dst_off floats (blocks of vp_mm_packed_bytes); vp_mm_pack_table packs n of them from
 * a DEVICE copy of the descriptor array. */
size_t vp_mm_packed_bytes(int P, int K, int N, int dir);
size_t vp_mm_pack_desc_bytes(void);
int vp_mm_pack_desc(size_t w_off, int ldw, int w_transposed, int P, int K, int N, int dir, size_t dst_off, void* desc);
int vp_mm_pack_table(const void* device_descs, int n, const float* master, void* packed, void* stream);
int vp_mm_fwd_f32_packed(const float* x, int ldx, const void* packed_w, const float* bias, float* y, int ldy, int P, int K, int N,
                         void* workspace, void* stream);
int vp_mm_bwd_data_f32_packed(const float* dy, int lddy, const void* packed_w, float* dx, int lddx, int accumulate, int P, int K, int N,
                              void* workspace, void* stream);

/* ---- cv2.resize(uint8, INTER_LINEAR) + paste: the last step of render_face (voicepuppet/pixrefer/infer_bfmvid.py:110-121) ----
 * OpenCV's fixed-point bilinear (11-bit coefficients, the two-pass rounding of resize.cpp: see csrc/resize.hip), byte for byte;
 * optionally behind cv2.cvtColor(BGR2RGB).  src [frames][src_h][src_w][3] uint8 is resized to dst_h x dst_w and written into
 * canvas [frames][canvas_h][canvas_w][3] at (y0, x0); canvas pixels outside the pasted rectangle are not touched (the caller zeroes
 * the canvas, as np.zeros does in the reference).  workspace: vp_resize_paste_workspace_bytes(dst_h, dst_w) device bytes.
 * vp_resize_linear_table: the coefficient tables alone (host arrays of dst_size entries), for host callers and tests. */
size_t vp_resize_paste_workspace_bytes(int dst_h, int dst_w);
int vp_resize_paste_u8(const unsigned char* src, int frames, int src_h, int src_w, int dst_h, int dst_w, int swap_rb,
                       unsigned char* canvas, int canvas_h, int canvas_w, int y0, int x0, void* workspace, void* stream);
int vp_resize_linear_table(int src_size, int dst_size, int rows, int* ofs, short* a0, short* a1, int* row1);

/* ------------------------------------------------------------------------------------------------
 * Frames for stream groups: the steps between a group push's packed expression coefficients and the generator's inputs, for rows of
 * up to VP_PUPPET_MAX_SLOTS talkers, each with its own photo, coefficients and paste geometry (voicepuppet_amd.stream.PuppetStreamGroup).
 * A handle owns the per-slot state in a caller-owned device workspace: photo coefficients [slots,257], the two float reference panels
 * [slots,H,H,3] each, the slot's cv2.resize tables.  attach may wait (once per talker); splice / condition only enqueue and read their
 * per-push tables from DEVICE memory (the caller stages them through pinned memory).
 *   vp_puppet_splice      replaces infer_bfmvid.py:223-224 (np.tile + np.concatenate of the photo's coefficients around the predicted
 *                         expression).  rows [count][4] int: {slot, row of expr, -, -}; coeff_out [count,257].  Copies only.
 *   vp_puppet_condition   replaces, for `count` <= frame_batch rows in ONE launch: render_face's cvtColor + cv2.resize + paste into a zero
 *                         canvas (infer_bfmvid.py:110-121), the caller's second channel swap and /255 (:233), the reference panels in
 *                         channels 0:3 of inputs / fg_inputs (:200-203, :229-230) and the background target of the row's global frame
 *                         index or 0.5 (:236-238).  rows [count][4] int: {slot, row of faces or -1, row of the background bank or -1,
 *                         global frame index}.  faces [face_rows][face_size][face_size][3] uint8 in rasteriser order.  A slot attached
 *                         without coefficients takes its reference panel for channels 3:6.  inputs [frame_batch,H,H,6], fg_inputs /
 *                         targets [frame_batch,H,H,3] float32; the uint8 -> float step gives the bits of the expression it replaces (csrc/puppet_cond.hip).
 *                         A row whose table entries are out of range is left unwritten.
 * ---------------------------------------------------------------------------------------------- */
#define VP_PUPPET_MAX_SLOTS 128
typedef struct vp_puppet_desc {
  int struct_bytes;       /* sizeof(vp_puppet_desc) of the caller's build: must equal vp_puppet_desc_size() */
  int slots;              /* 1 .. VP_PUPPET_MAX_SLOTS */
  int frame_batch;        /* rows per vp_puppet_condition launch (the generator plan's batch): 1 .. 1024 */
  int img_size;           /* H: a multiple of 256 (every image line is then whole 1 KB store runs) */
  int face_size;          /* side of the rasterised face images: 224 */
} vp_puppet_desc;
size_t vp_puppet_desc_size(void);
typedef struct vp_puppet vp_puppet_t;
/* 0 on a refused descriptor (vp_last_error says why) */
size_t vp_puppet_workspace_bytes(const vp_puppet_desc* d);
int vp_puppet_create(const vp_puppet_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_puppet_t** out);
void vp_puppet_destroy(vp_puppet_t* h);
/* refer / fg_refer: DEVICE float [H,H,3] (copied).  photo_coeff: HOST float [257], or NULL for a slot conditioned on its reference panel
 * (side / y0 / x0 are then ignored).  side: the face is resized to side x side (1 .. 4 * img_size) and pasted at (y0, x0); its
 * resize tables (vp_resize_linear_table) are built here, once. */
int vp_puppet_attach(vp_puppet_t* h, int slot, const float* refer, const float* fg_refer, const float* photo_coeff, int side, int y0, int x0,
                     void* stream);
/* bank: DEVICE uint8 [count,H,H,3], caller-owned, the backgrounds that exist (the table rows of vp_puppet_condition index it) */
int vp_puppet_set_backgrounds(vp_puppet_t* h, const unsigned char* bank, int count);
int vp_puppet_splice(vp_puppet_t* h, const float* expr, int expr_rows, const int* rows, int count, float* coeff_out, void* stream);
int vp_puppet_condition(vp_puppet_t* h, const unsigned char* faces, int face_rows, const int* rows, int count, float* inputs, float* fg_inputs,
                        float* targets, void* stream);
/* "coeff" [slots,257], "refer" / "fg" [slots,H,H,3]: the per-slot state in the workspace */
int vp_puppet_tensor(vp_puppet_t* h, const char* name, void** ptr, int64_t shape[4]);
/* Host only: info = {kind (0 empty, 1 reference panel, 2 copy, 3 exact 2x reduction, 4 bilinear), side, y0, x0} */
int vp_puppet_slot_info(const vp_puppet_t* h, int slot, int info[4]);

/* ------------------------------------------------------------------------------------------------
 * JPEG encoding of emitted frames on the device: replaces infer_bfmvid.py:243-244 (cv2.imwrite('output/{}.jpg') per frame, on the host)
 * for the uint8 RGB frames of a whole launch (Outputs_u8, PuppetStreamGroup.last_frames).  csrc/jpeg_enc.hip.
 *
 * The stream is a JFIF 1.01 baseline file: SOI, APP0 (density 1:1), DQT x 2, SOF0 (8 bit, height x width, Y 2x2, Cb 1x1, Cr 1x1), DHT x 4,
 * DRI, SOS, entropy-coded data with RSTn markers, EOI.  Colour: full-range YCbCr in float32 from the uint8 frame, not rounded; chroma the
 * mean of each 2 x 2; level shift 128; float32 8 x 8 DCT; the ITU T.81 Annex K quantisation tables scaled by libjpeg's quality rule
 * (quality 1 .. 100; 75 is what PIL's save() uses), quotient rounded to nearest, ties away from zero; the four Annex K Huffman tables;
 * restart interval = one MCU row (width / 16 MCUs), RSTn cycling 0 .. 7.
 *
 * Capacity rule.  Every restart interval (16 image rows) is coded into a slot of VP_JPEG_SLOT_BYTES(width) = 24 * width bytes of the
 * workspace: half the interval's raw RGB, 64 bytes per 8 x 8 block on average.  (Uniform random noise at quality 75 takes two fifths of
 * that in its largest interval, a photograph a tenth.)  An interval whose code, before or after byte stuffing, does not fit its slot is dropped: nothing is
 * written past a slot or past the caller's row, and out_bytes[frame] becomes -1; the caller encodes that frame on the host.
 * vp_jpeg_frame_capacity is header + (height / 16) * (slot + 2) + padding: a row of that many bytes holds every frame whose intervals fit.
 * ---------------------------------------------------------------------------------------------- */
#define VP_JPEG_MAX_FRAMES 4096
#define VP_JPEG_SLOT_BYTES(width) (24 * (width))
typedef struct vp_jpeg_desc {
  uint32_t struct_bytes;  /* sizeof(vp_jpeg_desc) of the caller's build: must equal vp_jpeg_desc_size() */
  int32_t max_frames;     /* frames per vp_jpeg_encode: 1 .. VP_JPEG_MAX_FRAMES */
  int32_t height;         /* multiples of 16 (4:2:0 MCUs), height up to 4096; width up to 832 (an MCU row's coefficients and bit */
  int32_t width;          /* buffer live in one workgroup's 64 KB of LDS); the product's sizes are 256 and 512 */
  int32_t quality;        /* 1 .. 100 */
} vp_jpeg_desc;
size_t vp_jpeg_desc_size(void);
typedef struct vp_jpeg vp_jpeg_t;
/* 0 on a refused descriptor (vp_last_error says why) */
size_t vp_jpeg_workspace_bytes(const vp_jpeg_desc* d);
size_t vp_jpeg_frame_capacity(const vp_jpeg_desc* d);
/* Builds the header and uploads the tables; may wait, once per encoder (replaces nothing per frame: cv2.imwrite, infer_bfmvid.py:243-244,
 * rebuilds its tables for every file) */
int vp_jpeg_create(const vp_jpeg_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_jpeg_t** out);
/* rgb: DEVICE uint8 [frames,height,width,3] on a 4-byte boundary, 1 .. max_frames frames.  out: DEVICE bytes, frame f's file starts at
 * out + f * out_row_bytes; out_bytes: DEVICE int [frames], the file's length or -1 (capacity rule above; rows f >= frames are not
 * touched).  Two launches on `stream`; never waits, never allocates.  Replaces the per-frame cv2.imwrite of infer_bfmvid.py:243-244. */
int vp_jpeg_encode(vp_jpeg_t* h, const unsigned char* rgb, int frames, unsigned char* out, size_t out_row_bytes, int* out_bytes, void* stream);
/* "coefficients": int16 [max_frames, height/16, 6 * width/16, 64], per MCU row the blocks in scan order (Y Y Y Y Cb Cr per MCU), zig-zag
 * inside a block, as quantised.  For tests: encodes store them from the first call of this function on (a second write of 1.5x the frame). */
int vp_jpeg_tensor(vp_jpeg_t* h, const char* name, void** ptr, int64_t shape[4]);
/* Host only: the bytes before the entropy-coded data (SOI .. SOS), *n their count; host_out may be NULL to ask for the count alone */
int vp_jpeg_header(const vp_jpeg_t* h, unsigned char* host_out, size_t cap, size_t* n);
void vp_jpeg_destroy(vp_jpeg_t* h);

/* ------------------------------------------------------------------------------------------------
 * Stream ingest: client PCM (interleaved int16 or float32, 1 .. 8 channels, any of up to 8 rates named at create) to the mono float32
 * out_rate signal vp_bfmstream_group_push takes, on the device and chunk by chunk.  Replaces, for live audio, the whole-file host
 * conversion of generator/loader.py:39-54 (WavLoader.get_data: scale, mean over the channels, scipy.signal.resample_poly).  csrc/pcm_in.hip.
 *
 *   convert   VP_PCM_S16: float32(v) / 32768.  VP_PCM_F32: as is.
 *   down-mix  1 channel: nothing.  2: (a + b) / 2 in float32.  3 .. 8: float32 sum left to right, one division by the count.
 *   resample  g = gcd(in_rate, out_rate), up = out_rate / g, down = in_rate / g.  up == down: a copy (no filter, no delay).  Else scipy's
 *             default design: half = 10 * max(up, down), h = float32(firwin(2 half + 1, 1 / max(up, down), ('kaiser', 5.0))) * up,
 *             y[m] = sum_k h[m down - k up + half] x[k], x zero outside the clip, m = 0 .. ceil(N up / down) - 1 for a clip of N frames:
 *             resample_poly(x, up, down).  Each y[m] is one float32 fma chain over the taps of its phase in a fixed order, so the bits of
 *             a clip's output do not depend on how pushes cut it, on the slot, or on the other slots of a push.
 *   emission  after n frames of a clip that has not finished: the outputs m with m down + half <= n up - 1 (every tap has arrived),
 *             at most ceil(n up / down); at finish all ceil(N up / down).  Host arithmetic (vp_pcmin_samples_after): a push never waits.
 *             The lookahead is half / up input frames = 10 output samples (0.625 ms) when downsampling.
 * A rate is accepted when its polyphase bank [up][ceil((2 half + 1) / up)] float32 is at most 1 MiB, up <= 65535 and one tile of 256
 * outputs reads at most 4096 input frames (all of 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000 and 192000
 * Hz to 16000 Hz are; 44101 Hz, 3.5 MB, is not).
 * ---------------------------------------------------------------------------------------------- */
#define VP_PCMIN_MAX_SLOTS 128
#define VP_PCMIN_MAX_CHANNELS 8
enum vp_pcm_format { VP_PCM_S16 = 0, VP_PCM_F32 = 1 };
typedef struct vp_pcmin_desc {
  int struct_bytes;       /* sizeof(vp_pcmin_desc) of the caller's build: must equal vp_pcmin_desc_size() */
  int slots;              /* 1 .. VP_PCMIN_MAX_SLOTS */
  int out_rate;           /* 16000 */
  int max_in_frames;      /* input frames per slot and push: 1 .. 4194304 (lane offsets are 32-bit; callers split longer chunks) */
  int n_rates;            /* 1 .. 8 */
  int rates[8];           /* the input rates slots may be opened with, each once */
} vp_pcmin_desc;
size_t vp_pcmin_desc_size(void);
typedef struct vp_pcmin vp_pcmin_t;
/* Host only, no handle.  vp_pcmin_ratio: up, down, half and the taps per phase (any may be NULL); up == down gives half 0, 1 tap.
 * vp_pcmin_bank: h[2 half + 1] as above (h[0] = 1 for up == down).  vp_pcmin_samples_after: the emission rule, -1 on a bad argument. */
int vp_pcmin_ratio(int in_rate, int out_rate, int* up, int* down, int* half, int* taps_per_phase);
int vp_pcmin_bank(int in_rate, int out_rate, float* h);
long long vp_pcmin_samples_after(int in_rate, int out_rate, long long in_frames, int finished);
/* 0 on a refused descriptor (vp_last_error names the field) */
size_t vp_pcmin_workspace_bytes(const vp_pcmin_desc* d);
/* Designs the filters and uploads their banks; may wait, once per handle */
int vp_pcmin_create(const vp_pcmin_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_pcmin_t** out);
void vp_pcmin_destroy(vp_pcmin_t* h);
/* Slot `slot` starts a clip of in_rate (one of the descriptor's), `channels` interleaved channels of `format`; also restarts an open slot.
 * Enqueues the clearing of the slot's history on `stream`; does not wait. */
int vp_pcmin_open_slot(vp_pcmin_t* h, int slot, int in_rate, int channels, int format, void* stream);
/* Host only: out_samples[s] (may be NULL) a push of in_frames[s] new frames per slot emits, finish[s] != 0 ending slot s's clip after them
 * (finish may be NULL); returns the sum, or -1 (frames or finish for a slot that is not open or has finished, a count outside
 * 0 .. max_in_frames) */
long long vp_pcmin_ready(const vp_pcmin_t* h, const long long* in_frames, const int* finish, long long* out_samples);
/* raw: DEVICE bytes on a 16-byte boundary, the slots' new frames packed in slot order: slot s's segment is in_frames[s] * channels * sample
 * bytes long and starts at the next 16-byte boundary after the previous one.  pcm_out: DEVICE float32, the slots' new samples packed in
 * slot order - the pcm argument of vp_bfmstream_group_push with n[s] = out_samples[s].  One launch on `stream`; never waits, never allocates. */
int vp_pcmin_push(vp_pcmin_t* h, const void* raw, const long long* in_frames, const int* finish, float* pcm_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG encoding of device tensors: replaces the host PNG encode behind the reference's image summaries (train_pixrefer.py:105-118: five
 * tf.summary.image calls, up to three images each, every summary step) for the frames of a whole launch.  csrc/png_enc.hip; the byte
 * stream is restated in tests/png_ref.py, which is its definition.
 *
 * Source: a DEVICE tensor [frames, height, width, pixel_stride], uint8 or float32, of which `channels` components starting at
 * channel_offset are encoded in place (Inputs[..., 3:6] of the 6-channel training input needs no slice copy).  uint8 passes through.
 * float32 follows tf.image.convert_image_dtype(x, tf.uint8): (uint8) trunc(x * 255.5f).  Outside [0, 1] the reference's unsaturated cast
 * is undefined; here values below 0 and NaN give 0, values from 255 / 255.5 up give 255.
 *
 * The file is PNG 1.2, bit depth 8, colour type 0 / 2 / 6 (1 / 3 / 4 channels), no interlace: signature, IHDR, IDAT(78 01), one IDAT
 * per strip, IDAT(03 00, Adler-32), IEND.  A strip is R = vp_png_rows_per_strip rows: the largest R <= 16 with
 * (2 R + 1) * width * channels + R + 32 <= 53248, so that a strip's raw rows, filtered bytes and bit buffer fit one workgroup's LDS;
 * width * channels is therefore at most VP_PNG_MAX_ROW_BYTES (R = 1).  Per strip: PNG filters (filter -1: per row the one with the
 * smallest sum of absolute signed residuals, the lowest number on a tie; 0 .. 4: that filter on every row), literals and runs (matches
 * at distance 1, 3 .. 258 long; no other LZ77), one dynamic-Huffman block (length limits 15 / 7, no repeat symbols, one distance code)
 * closed by an empty stored block as zlib's sync flush writes it, or, when that is not shorter, one stored block and the empty one.
 *
 * Capacity.  A stored strip takes its filtered bytes + 22, so a file's size has a bound that depends on the descriptor alone:
 * vp_png_frame_capacity (47 + sum over strips (rows * (1 + width * channels) + 22) + 30, rounded up to 256).  There is no "did not fit".
 * ---------------------------------------------------------------------------------------------- */
#define VP_PNG_MAX_FRAMES 4096
#define VP_PNG_MAX_HEIGHT 65535
#define VP_PNG_MAX_ROW_BYTES 17738
#define VP_PNG_MAX_PIXEL_STRIDE 64
enum vp_png_dtype { VP_PNG_U8 = 0, VP_PNG_F32 = 1 };
typedef struct vp_png_desc {
  uint32_t struct_bytes;  /* sizeof(vp_png_desc) of the caller's build: must equal vp_png_desc_size() */
  int32_t max_frames;     /* frames per vp_png_encode: 1 .. VP_PNG_MAX_FRAMES */
  int32_t height;         /* 1 .. VP_PNG_MAX_HEIGHT */
  int32_t width;          /* width * channels: 1 .. VP_PNG_MAX_ROW_BYTES */
  int32_t channels;       /* 1 (grey), 3 (RGB) or 4 (RGBA) */
  int32_t filter;         /* -1 adaptive (the default), 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth on every row */
} vp_png_desc;
size_t vp_png_desc_size(void);
typedef struct vp_png vp_png_t;
/* 0 on a refused descriptor (vp_last_error says why) */
size_t vp_png_workspace_bytes(const vp_png_desc* d);
size_t vp_png_frame_capacity(const vp_png_desc* d);
int vp_png_rows_per_strip(const vp_png_desc* d);
/* Host only apart from one upload (the 47 bytes before the strips); may wait, once per encoder */
int vp_png_create(const vp_png_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_png_t** out);
/* src: see above (src_dtype a vp_png_dtype; float32 on a 4-byte boundary; channel_offset + channels <= pixel_stride <=
 * VP_PNG_MAX_PIXEL_STRIDE), 1 .. max_frames frames.  out: DEVICE bytes, frame f's file starts at out + f * out_row_bytes, out_row_bytes
 * at least the capacity rule's bound; out_bytes: DEVICE int [frames], the file's length (rows f >= frames are not touched).  Two launches
 * on `stream`; never waits, never allocates; a bad argument is refused with VP_ERR_ARG before anything is enqueued.  Replaces the PNG
 * encodes of train_pixrefer.py:105-118. */
int vp_png_encode(vp_png_t* h, const void* src, int src_dtype, int pixel_stride, int channel_offset, int frames, unsigned char* out,
                  size_t out_row_bytes, int* out_bytes, void* stream);
/* "strips": int32 [max_frames, strips, 4, 1] of the last encode: the strip's IDAT chunk bytes, its Adler-32 a and b, 1 when stored */
int vp_png_tensor(vp_png_t* h, const char* name, void** ptr, int64_t shape[4]);
/* Host only: the bytes before the first strip (signature, IHDR, IDAT(78 01)), *n their count; host_out may be NULL to ask for the count */
int vp_png_header(const vp_png_t* h, unsigned char* host_out, size_t cap, size_t* n);
void vp_png_destroy(vp_png_t* h);

/* ------------------------------------------------------------------------------------------------
 * JPEG decoding of training frames on the device: replaces the two cv2.imread calls per sample of generator/generator.py:956-1019 and
 * generator/loader.py's ImageLoader (a host libjpeg decode per file) for the files of a whole batch.  csrc/jpeg_dec.hip.
 *
 * Accepted: baseline sequential Huffman (SOF0), 8 bit, three components in one interleaved scan, sampling 4:2:0 (2x2, 1x1, 1x1) or 4:4:4
 * (and 4:2:2 on request, below),
 * any width and height up to the descriptor's, up to four 8-bit quantisation tables and two DC + two AC Huffman tables from the file, any
 * restart interval.  The host parses the headers (voicepuppet_amd/jpeg_dec.py::parse) and refuses the rest before anything is enqueued.
 *
 * The output is defined in integers, libjpeg's default decode (what PIL runs): dequantise; the "islow" inverse DCT (13-bit constants, two
 * passes, descale by 11 and 18, +128, clamp); for 4:2:0 "fancy" triangle up-sampling of chroma (3:1 vertically, then 3:1 horizontally with
 * +8 / +7 rounding on even / odd columns, the edge sample replicated at the border of the component's own ceil(W/2) x ceil(H/2) samples);
 * R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16) with
 * C' = C - 128, clamped.  All of it int32 (wrapping, which only coefficients no encoder writes can reach).  tests/jpeg_dec_ref.py restates it.
 *
 * 4:2:2 (sampling 3: components 2x1, 1x1, 1x1; what capture cards and Motion-JPEG encoders write) is taken when the caller passes it:
 * parse() refuses it unless asked (accept_422).  An MCU is 16 x 8 pixels and has four blocks in scan order Y0 (left), Y1 (right), Cb, Cr;
 * mcux = ceil(W / 16), mcuy = ceil(H / 8); a chroma component's own size is ceil(W / 2) x H.  Entropy decode, dequantisation, inverse DCT and
 * colour conversion are the ones above.  Up-sampling is libjpeg's h2v1 "fancy" triangle filter along the row only: of a chroma row
 * c[0 .. cw - 1], cw = ceil(W / 2), out[2i] = (3 c[i] + c[i-1] + 1) >> 2 and out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2 with c[-1] = c[0] and
 * c[cw] = c[cw-1] (the edge sample replicated at the border of the component's own samples, which gives libjpeg's unfiltered first and
 * last output samples, also for cw == 1); nothing is filtered down the column.  tests/jpeg_dec_422_ref.py restates it.  The workspace is
 * the same: the padded sizes are multiples of 16, so 16 mcux and 8 mcuy fit them, and a 4:2:2 file has two thirds of the 4:4:4 blocks.
 *
 * Per-file meta blob (little endian, 16-byte aligned, VP_JPEGDEC_META_BYTES + 24 * n_segments bytes):
 *   [0, 128)       reserved for the host (the device reads none of it: what it needs of the header travels in vp_jpegdec_file)
 *   [128, 640)     uint16 quant[4][64], row-major inside a block
 *   [640, 6336)    four Huffman tables (DC 0, DC 1, AC 0, AC 1) of 1424 bytes: uint16 lut[512], entry (length << 8) | symbol of the code
 *                  that the next 9 bits start with, 0 when that code is longer; int32 maxcode[18] by length (-1: none); int32
 *                  valoff[18], symbol index = code + valoff[length]; uint8 vals[256]
 *   [6336, ...)    int32 segments[n][6]: byte offset in the file of the byte that holds the segment's first bit; that bit (0 = most
 *                  significant); DC predictors Y | Cb << 16; predictor Cr; first MCU; MCU count.  A segment may be any run of MCUs: a
 *                  restart boundary inside it is crossed at its marker.
 * "entries" [max_files][mcu rows][4] int32: the first four of those fields as a lane met them at every MCU-row start: fed back as segments
 * (first MCU = row * MCUs per row) they decode a file without restart markers with one lane per MCU row.
 * ---------------------------------------------------------------------------------------------- */
#define VP_JPEGDEC_MAX_FILES 4096
#define VP_JPEGDEC_META_BYTES 6336
#define VP_JPEGDEC_FILES_PER_LAUNCH 32
typedef struct vp_jpegdec_desc {
  uint32_t struct_bytes;          /* sizeof(vp_jpegdec_desc) of the caller's build: must equal vp_jpegdec_desc_size() */
  int32_t max_files;              /* files per vp_jpegdec_decode: 1 .. VP_JPEGDEC_MAX_FILES */
  int32_t max_height;             /* 1 .. 8192 */
  int32_t max_width;              /* 1 .. 8192 */
  int32_t max_file_bytes;         /* 1 .. 2^30 */
  int32_t max_segments_per_file;  /* 1 .. 2^20 */
  int32_t bgr;                    /* 0: R G B byte order, 1: B G R (what vp_pixrefer_pack_frames takes) */
} vp_jpegdec_desc;
typedef struct vp_jpegdec_file {
  uint64_t meta_offset;           /* of the file's meta blob in `blob`, a multiple of 16 */
  uint64_t file_offset;           /* of the file's bytes in `blob` */
  int32_t file_bytes;
  int32_t width, height;
  int32_t sampling;               /* 2: 4:2:0, 1: 4:4:4, 3: 4:2:2 */
  int32_t restart_interval;       /* MCUs, 0: none */
  int32_t n_segments;
  uint8_t tq[3], td[3], ta[3];    /* per component: quantisation table 0 .. 3, DC table 0 .. 1, AC table 0 .. 1 */
  uint8_t reserved[3];
} vp_jpegdec_file;
size_t vp_jpegdec_desc_size(void);
typedef struct vp_jpegdec vp_jpegdec_t;
/* 0 on a refused descriptor (vp_last_error names the field) */
size_t vp_jpegdec_workspace_bytes(const vp_jpegdec_desc* d);
/* Host only: touches no device memory.  Replaces nothing per file (ImageLoader, generator/loader.py, sets libjpeg up for every file) */
int vp_jpegdec_create(const vp_jpegdec_desc* d, void* workspace, size_t workspace_bytes, vp_jpegdec_t** out);
void vp_jpegdec_destroy(vp_jpegdec_t* h);
/* blob: DEVICE bytes, metas and files as packed by the host, on a 16-byte boundary.  files: HOST, n entries, read before the call returns:
 * the per-file table travels as kernel arguments, VP_JPEGDEC_FILES_PER_LAUNCH files per group of three launches (entropy, planes, rgb).
 * out: DEVICE uint8, file f's pixel (y, x) at out + f * frame_stride + y * row_pitch + 3 x; only the file's own width x height pixels are
 * written.  status: DEVICE int [n], 0 or -1 (a lane ran out of data, met an invalid code or a missing restart marker, or overran a block).
 * A file with n_segments == 0 is a gap: its other fields are ignored, nothing is read or written for its position (a row the caller fills
 * itself, a file the host parser refused), its status is 0.
 * Enqueues on `stream`; never waits, never allocates.  Replaces the cv2.imread pair of generator/generator.py:956-1019 and ImageLoader. */
int vp_jpegdec_decode(vp_jpegdec_t* h, const unsigned char* blob, const vp_jpegdec_file* files, int n, unsigned char* out, size_t row_pitch,
                      size_t frame_stride, int* status, void* stream);
/* "coefficients": int16 [max_files, blocks, 64], the blocks of a file in scan order, row-major inside a block, as decoded (not dequantised).
 * "entries": int32 [max_files, mcu rows, 4].  "planes": uint8 [max_files, 3, padded height, padded width] (Y, Cb, Cr; chroma of a 4:2:0
 * file fills the top left quarter; chroma of a 4:2:2 file fills the left half).  Rows of the first axis are positions in the last decode call. */
int vp_jpegdec_tensor(vp_jpegdec_t* h, const char* name, void** ptr, int64_t shape[4]);
/* Device index scan (opt-in): finds the MCU-row entry points of a file without restart markers inside the decode call that first sees
 * it, so that this very call already runs one lane per MCU row.  One workgroup per file cuts the entropy-coded segment into chunks of
 * chunk_bytes raw file bytes, decodes every chunk from a guessed state, and repeats "chunk i from the exit state of chunk i - 1" until a
 * round changes nothing (Huffman streams self-synchronise; Weissenberger & Schmidt, ICPP 2018); a prefix sum over block counts and DC
 * differences then gives the block index and the predictors at every chunk start, and one more walk writes "entries".
 * chunk_bytes: a power of two, 32 .. 4096.  max_rounds: 1 .. 1024, the bound on the fixed-point rounds of one sweep (a sweep: as many
 * chunks as the workgroup has lanes).  vp_jpegdec_scan_workspace_bytes returns 0 on a refused value (vp_last_error names it).
 * vp_jpegdec_enable_scan is host only; scan_workspace is DEVICE memory the caller keeps alive as long as the decoder.  Without this call
 * vp_jpegdec_decode is unchanged.  With it, a file is scanned when n_segments == 1, restart_interval == 0, it has at least two MCU rows
 * and its one segment starts at MCU 0 and covers every MCU; every other file of the call takes the usual path.  The scan holds
 * ("scan_ok" 1) only if the rounds settled, no settled lane met an invalid code and the block total is the file's; otherwise one lane
 * decodes the file's single segment as without the scan.  Two more names of vp_jpegdec_tensor, both int32 [max_files] and 0 for a file
 * that was not scanned: "scan_ok", and "scan_rounds", the most rounds a sweep of the file took (the last, unchanged round included). */
size_t vp_jpegdec_scan_workspace_bytes(const vp_jpegdec_desc* d, int chunk_bytes);
int vp_jpegdec_enable_scan(vp_jpegdec_t* h, void* scan_workspace, size_t scan_workspace_bytes, int chunk_bytes, int max_rounds);

/* ------------------------------------------------------------------------------------------------
 * Frame quality metrics on the device: per frame pair mean |a - b|, mean (a - b)^2, PSNR and SSIM of two batches of three-channel NHWC
 * (interleaved) frames that are already on the device (decoded dataset frames, generator output, emitted uint8 frames).  The reference has
 * no counterpart.  csrc/frame_metrics.hip; tests/frame_metrics_ref.py restates the definition in float64 numpy.
 *
 * Values are in [0, 255]: uint8 as is; float32 x mapped v = min(max(x * scale + offset, 0), 255) in double, no rounding (scale = offset =
 * 127.5 takes the generator's [-1, 1] output; a NaN maps to 0).
 *   L1    sum |a - b| / (3 H W)
 *   MSE   sum (a - b)^2 / (3 H W)
 *   PSNR  10 log10(255^2 / MSE) dB, +inf at MSE == 0
 *   SSIM  Wang, Bovik, Sheikh & Simoncelli 2004, per channel on the values in [0, 255].  Window: 11 x 11 Gaussian of sigma 1.5, the outer
 *         product of the 11-tap vector g[i] = exp(-(i - 5)^2 / (2 sigma^2)) normalised to sum 1 (computed in double on the host and
 *         handed to the kernel).  Per window, with E[.] the weighted mean: mu_a = E[a], mu_b = E[b], var_a = E[a^2] - mu_a^2,
 *         var_b = E[b^2] - mu_b^2, cov = E[a b] - mu_a mu_b (weighted population moments, no Bessel factor);
 *         S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
 *         Only the (H - 10) x (W - 10) windows that lie wholly inside the image; SSIM is the mean of S over those windows and the three
 *         channels.  This is skimage.metrics.structural_similarity(a, b, gaussian_weights=True, use_sample_covariance=False,
 *         data_range=255, channel_axis=-1).  height < 11 or width < 11 is refused.
 * Arithmetic: all moments and S in float64 (E[x^2] - mu^2 cancels at 65025 against C2 = 58.5).  For uint8 input sum |a - b| and
 * sum (a - b)^2 are integers and exact.  No floating-point atomics: one workgroup per tile of 16 x 16 windows and frame writes its partial
 * sums to the workspace, a second kernel adds a frame's tiles in a fixed order (lane l of 256 adds tiles l, l + 256, ... in index order,
 * then a fixed tree over the lanes), so a frame's numbers depend on neither scheduling nor the other frames of the call.
 * ---------------------------------------------------------------------------------------------- */
#define VP_FRAME_METRICS_MAX_FRAMES 4096
typedef struct vp_frame_metrics_desc {
  uint32_t struct_bytes;          /* sizeof(vp_frame_metrics_desc) of the caller's build: must equal vp_frame_metrics_desc_size() */
  int32_t max_frames;             /* frame pairs per call: 1 .. VP_FRAME_METRICS_MAX_FRAMES */
  int32_t max_height;             /* 11 .. 8192 */
  int32_t max_width;              /* 11 .. 8192 */
} vp_frame_metrics_desc;
size_t vp_frame_metrics_desc_size(void);
typedef struct vp_frame_metrics vp_frame_metrics_t;
/* 0 on a refused descriptor (vp_last_error names the field) */
size_t vp_frame_metrics_workspace_bytes(const vp_frame_metrics_desc* d);
/* Host only: touches no device memory.  workspace: DEVICE memory the caller keeps alive as long as the handle. */
int vp_frame_metrics_create(const vp_frame_metrics_desc* d, void* workspace, size_t workspace_bytes, vp_frame_metrics_t** out);
void vp_frame_metrics_destroy(vp_frame_metrics_t* h);
/* a, b: DEVICE uint8, frame f's value (y, x, c) at p + f * frame_stride + y * row_pitch + 3 x + c; pitches and strides in bytes and
 * independent for the two operands (a padded vp_jpegdec_decode output against a dense tensor).  Only the n x height x width x 3 values
 * are read.  out: DEVICE float64 [n][4]: L1, MSE, PSNR, SSIM.  Refused, before anything is enqueued (vp_last_error names the reason):
 * n outside 1 .. max_frames, height or width under 11 or over the descriptor's, row_pitch < 3 * width, frame_stride <
 * (height - 1) * row_pitch + 3 * width, more than 2^23 tiles of 16 x 16 windows in one call (64 frames of 8192 x 8192: split the batch).
 * Also refused: out off an 8-byte boundary, a row_pitch over 2^40 or a frame_stride over 2^48 bytes.
 * Two launches on `stream`; never waits, never allocates. */
int vp_frame_metrics_u8(vp_frame_metrics_t* h, const unsigned char* a, size_t a_row_pitch, size_t a_frame_stride, const unsigned char* b,
                        size_t b_row_pitch, size_t b_frame_stride, int n, int height, int width, double* out, void* stream);
/* The same for float32 elements (pointers, pitches and strides multiples of 4 bytes, a row 12 * width bytes), mapped as above. */
int vp_frame_metrics_f32(vp_frame_metrics_t* h, const float* a, size_t a_row_pitch, size_t a_frame_stride, const float* b, size_t b_row_pitch,
                         size_t b_frame_stride, int n, int height, int width, double scale, double offset, double* out, void* stream);
/* "abs_sum", "sq_sum": int64 [max_frames], sum |a - b| and sum (a - b)^2 of the frames of the last vp_frame_metrics_u8 call (a
 * vp_frame_metrics_f32 call leaves them alone).  shape[0] = max_frames. */
int vp_frame_metrics_tensor(vp_frame_metrics_t* h, const char* name, void** ptr, int64_t shape[4]);

/* ------------------------------------------------------------------------------------------------
 * AVI segments on the device: replaces infer_bfmvid.py:245 (ffmpeg over output/%d.jpg and the wav) for the JPEG rows of vp_jpeg_encode and
 * the 16 kHz float32 samples of a push.  The container is AVI 1.0 (RIFF 'AVI '): Motion-JPEG video chunks `00dc`, 16-bit PCM audio chunks
 * `01wb`, an `idx1` index; the host writes the headers and the index (voicepuppet_amd/avi.py AviWriter), the device the chunks.
 * csrc/avi_mux.hip.
 *
 * A call writes one blob, little-endian throughout:
 *   uint32 head[4]             table_bytes, used_bytes (table and every status-0 segment: the prefix worth copying), chunks, worst status
 *   uint32 slot[slots][4]      offset of the slot's segment from the start of the blob, its bytes, its chunks, its status
 *   uint32 entry[chunks][4]    AVIOLDINDEX entries in segment order (slot s's entries follow those of the slots before it): ckid, flags
 *                              0x10, offset of the chunk header from the start of the slot's segment, payload bytes
 *   (table_bytes = 16 + 16 * slots + 16 * (frames + slots) of the call: vp_avimux_table_bytes)
 *   the segments, in slot order.  A slot with samples or frames in the call has one contiguous segment: a `01wb` chunk first when it has
 *   samples (fourcc, uint32 payload bytes, int16 samples), then one `00dc` chunk per frame of the slot in row order (fourcc, uint32
 *   lengths[r], the bytes, one zero byte when lengths[r] is odd).  A segment's bytes and its entries do not depend on the other slots.
 * A sample x becomes clamp(rintf(x * 32768.0f), -32768, 32767), round half to even, NaN 0: what arrived as int16 / 32768 leaves as it came.
 * Status: 0 ok; 1 a frame of the slot has lengths[r] < 0 (vp_jpeg_encode's capacity rule): nothing is written for the slot (0 bytes, 0
 * chunks) and the host builds its segment; 2 the segment would end past out_capacity: offset, bytes, chunks and entries are what they
 * would be, and nothing of the segment is written.
 * Bounds: a row is read up to min(lengths[r], row_bytes); the samples of all slots together inside [0, samples) (counts are cut, in slot
 * order, to what is left of `samples`; offsets moved inside); writes inside [0, out_capacity).  Rows whose frame_slot is outside 0 ..
 * slots - 1 are left out; frame_slot must be non-decreasing (an unsorted one loses rows but breaks no bound).
 * ---------------------------------------------------------------------------------------------- */
#define VP_AVIMUX_MAX_FRAMES 4096
#define VP_AVIMUX_MAX_SLOTS 128
typedef struct vp_avimux_desc {
  uint32_t struct_bytes;  /* sizeof(vp_avimux_desc) of the caller's build: must equal vp_avimux_desc_size() */
  int32_t max_frames;     /* JPEG rows per call: 1 .. VP_AVIMUX_MAX_FRAMES */
  int32_t row_bytes;      /* the largest row pitch a call may pass (vp_jpeg_frame_capacity) */
  int32_t slots;          /* 1 .. VP_AVIMUX_MAX_SLOTS */
  int32_t max_samples;    /* samples of all slots per call */
} vp_avimux_desc;
size_t vp_avimux_desc_size(void);
typedef struct vp_avimux vp_avimux_t;
/* 0 on a refused descriptor (vp_last_error says why; one whose vp_avimux_out_capacity is 4 GiB or more is refused: offsets are 32 bits) */
size_t vp_avimux_workspace_bytes(const vp_avimux_desc* d);
/* table + max_frames * (8 + row_bytes + 1) + slots * 8 + 2 * max_samples: a blob of that many bytes never has status 2 */
size_t vp_avimux_out_capacity(const vp_avimux_desc* d);
/* the table's bytes for a call of `frames` rows (0 .. max_frames): where the first segment starts */
size_t vp_avimux_table_bytes(const vp_avimux_desc* d, int frames);
/* Host only: touches no device memory.  workspace: DEVICE memory the caller keeps alive as long as the handle. */
int vp_avimux_create(const vp_avimux_desc* d, void* workspace, size_t workspace_bytes, vp_avimux_t** out);
/* data [frames, row_bytes] bytes, lengths [frames] int, as vp_jpeg_encode writes them; frame_slot [frames] int, non-decreasing; pcm
 * [samples] float32 on a 4-byte boundary, slot s's samples at sample_offset[s] .. + sample_count[s] (int [slots] each; the packed layout
 * of vp_bfmstream_group_push); out: the blob, on a 4-byte boundary, out_capacity bytes.  All of these DEVICE memory; frames (0 ..
 * max_frames) and samples (0 .. max_samples) are host counts and may be 0, the pointers of an empty half NULL.  Two launches on `stream`
 * (the table and the chunk list; the copies and the sample conversion); never waits, never allocates.  Calls on one handle must be
 * ordered (one stream, or events): the chunk list lives in the workspace. */
int vp_avimux_segment(vp_avimux_t* h, const unsigned char* data, size_t row_bytes, const int* lengths, const int* frame_slot, int frames,
                      const float* pcm, const int* sample_offset, const int* sample_count, int samples, unsigned char* out, size_t out_capacity,
                      void* stream);
void vp_avimux_destroy(vp_avimux_t* h);

/* ------------------------------------------------------------------------------------------------
 * PixReferNet training triptychs on the device: [frame | 3-D face on the frame | mask], the file generator/generator.py:924-1040 reads.
 * Replaces the image part of step 5 of datasets/make_data_from_GRID.py (deep_video_portraits, :430-469) and, with an alpha matte, the
 * layout of step 6 (:690-695), for all frames of a call.  csrc/triptych.hip.  Per frame, with face = face_size:
 *   a  filled = scipy.ndimage.binary_fill_holes(face_mask > 0), default structuring element (:431-433): a zero pixel is filled unless a
 *      4-connected path of zero pixels joins it to the image border.
 *   b  cv2.resize(filled as 0/1 float32, (side, side)), INTER_LINEAR (:435-436): f = (d + 0.5) * (face / side) - 0.5 in double, s = floor(f),
 *      fraction f - s; s < 0: s = 0, fraction 0; s >= face - 1: s = face - 1, fraction 0; the coefficients (1 - fraction, fraction) cast to
 *      float32; the horizontal pass, then the vertical pass, each v0 * c0 + v1 * c1 in float32, every product and sum rounded on its own.
 *   c  cv2.erode with np.ones((5, 5)) (:438-439): the minimum over the 5 x 5 window centred on the pixel, pixels outside the image left out.
 *   d  u = (uint8)(m * 255), truncated, then cv2.GaussianBlur(u, (21, 21), cv2.BORDER_DEFAULT) (:441): the reference passes the constant 4
 *      in the sigma position, so sigmaX = sigmaY = 4 and the border is the default REFLECT_101.  Defined here in integers: q[k] =
 *      round(65536 * g[k]) with g the normalised exp(-(k - 10)^2 / 32) in double, the centre tap adjusted so that the taps sum to 65536
 *      (vp_triptych_blur_taps); the horizontal sums in 32 bits, the vertical sums in 64, the result (v + 2^31) >> 32.  OpenCV's own
 *      uint8 Gaussian has coarser fixed-point taps: about +-1 grey level from this one (equality with cv2 is not claimed for b-d).
 *   e  paste at rows y0.., columns x0.. of a size x size canvas of zeros: the mask as float32(u) / 255 (:442, :457-458), and the render
 *      behind cv2.cvtColor(BGR2RGB) and cv2.resize(uint8, (side, side)) (:444-446, :449-455) - the bytes of vp_resize_paste_u8 with swap_rb.
 *   f  panels in float32, every operation rounded on its own, truncated to uint8 (:460-469): the frame; (frame * (1 - m) + face * m) *
 *      (m > 0); m * 255 on the three channels.
 *   g  with alpha: the frame; the pasted render on black; alpha on the three channels (:692-695).  Stages a-d are skipped.
 * Geometry (side, y0, x0) is the caller's; the Python layer takes it from infer_bfmvid.paste_geometry, that is step 6's and inference's
 * int() (infer_bfmvid.py:83-86), NOT step 5's int(round()) (:397-398): training sees the paste that inference produces.
 * Status per frame: 0 built; 1 side < 11 (REFLECT_101 of 21 taps); 2 side > max_side; 3 the paste rectangle is not wholly inside the canvas
 * (the reference's numpy assignment raises there).  A frame with a nonzero status leaves its triptych bytes untouched; nothing is read or
 * written out of bounds for any table contents.
 * ---------------------------------------------------------------------------------------------- */
#define VP_TRIPTYCH_MAX_FRAMES 4096
#define VP_TRIPTYCH_MAX_SIZE 1024
typedef struct vp_triptych_desc {
  uint32_t struct_bytes;  /* sizeof(vp_triptych_desc) of the caller's build: must equal vp_triptych_desc_size() */
  int32_t max_frames;     /* frames per call: 1 .. VP_TRIPTYCH_MAX_FRAMES */
  int32_t size;           /* the square canvas S: 11 .. VP_TRIPTYCH_MAX_SIZE */
  int32_t face_size;      /* the render and its mask: 2 .. 256 (224) */
  int32_t max_side;       /* the largest side a frame may ask for: 11 .. size */
} vp_triptych_desc;
size_t vp_triptych_desc_size(void);
typedef struct vp_triptych vp_triptych_t;
/* 0 on a refused descriptor (vp_last_error says why) */
size_t vp_triptych_workspace_bytes(const vp_triptych_desc* d);
/* Builds the resize tables of every side 1 .. max_side and uploads them; may wait, once per builder */
int vp_triptych_create(const vp_triptych_desc* d, void* workspace, size_t workspace_bytes, void* stream, vp_triptych_t** out);
/* All DEVICE pointers, n = 1 .. max_frames frames: frames uint8 [n,size,size,3] RGB; render uint8 [n,face,face,3] in the rasteriser's channel
 * order (vp_bfm_reconstruct_view); face_mask uint8 [n,face,face] (may be NULL with alpha); geometry int32 [n,3] = (side, y0, x0); alpha
 * NULL or uint8 [n,size,size]; triptych uint8 [n,size,3*size,3]; status int32 [n].  Six launches on `stream` (one with alpha); never waits,
 * never allocates.  Replaces make_data_from_GRID.py:430-469 per frame (:692-695 with alpha). */
int vp_triptych_build(vp_triptych_t* h, const unsigned char* frames, const unsigned char* render, const unsigned char* face_mask, const int* geometry,
                      const unsigned char* alpha, int n, unsigned char* triptych, int* status, void* stream);
/* Stages a-d alone (fill != 0) or b-d on face_mask > 0 as it is (fill == 0), into the "mask" planes; frames with a nonzero status are skipped */
int vp_triptych_mask(vp_triptych_t* h, const unsigned char* face_mask, const int* geometry, int n, int fill, void* stream);
/* Stage a alone, no handle: masks uint8 [n,height,width] (DEVICE, height and width 1 .. 256) -> out uint8 [n,height,width] of 0 / 1.
 * One workgroup per mask, rounds of row and column passes over two bitmaps in LDS until nothing changes (:431-433). */
int vp_triptych_fill_holes(const unsigned char* masks, int n, int height, int width, unsigned char* out, void* stream);
/* Host only: the 21 integer taps of stage d */
int vp_triptych_blur_taps(int q[21]);
/* "mask": uint8 [max_frames, max_side, max_side], the blurred mask u of the last build or vp_triptych_mask in its top-left side x side
 * corner; "filled": uint8 [max_frames, face_size, face_size], stage a's 0 / 1 */
int vp_triptych_tensor(vp_triptych_t* h, const char* name, void** ptr, int64_t shape[4]);
void vp_triptych_destroy(vp_triptych_t* h);

/* ------------------------------------------------------------------------------------------------
 * Alpha mattes for clips in front of a plain backdrop, on the device: a colour model of the backdrop fitted to the frames' border, a soft
 * key on the distance from it, one guided-filter pass (He, Sun & Tang 2010) with the frame's luma as the guide.  In place of the matte
 * that step 6 of datasets/make_data_from_GRID.py pastes from its segmentation and matting networks (:690-695), for a head and shoulders
 * in front of a studio backdrop only.  It is a key, not a matting network: on a cluttered background it is the wrong tool, and the
 * model's status, kept and residual_rms say so.  No spill suppression, no temporal smoothing.  csrc/key_matte.hip.
 *
 * Frames are uint8 RGB, frame f's value (y, x, c) at p + f * frame_stride + y * row_pitch + 3 x + c, 16 <= height, width <= 1024.
 * Everything below is integers or float64, every product, quotient and sum rounded on its own (no fused multiply-add) and in the order
 * written: parentheses first, otherwise left to right.  (double) of an integer is the nearest double.
 *
 * FIT.  Samples: the pixels with y < band, or with y < side_rows and (x < band or x >= W - band): the top and the upper sides (the torso
 *   leaves through the bottom).  band = 0 means max(2, H / 16), side_rows = 0 means H / 2 (integer divisions); refused unless
 *   1 <= band, 2 * band <= W and band <= side_rows <= H.  Per sample v = (x, y, R, G, B, 1) in integers; the moments are the 21 entries
 *   v[i] * v[j], i <= j, summed over the samples of all n frames in int64 (exact in any order), stored row by row of the upper triangle:
 *   xx xy xR xG xB x | yy yR yG yB y | RR RG RB R | GG GB G | BB B | 1  (indices 0..5, 6..10, 11..14, 15..17, 18..19, 20).
 *   Pass 1: the moments of all samples, then SOLVE.  Pass 2: the moments of the samples whose d2 (APPLY, with pass 1's model) is <= trim,
 *   then SOLVE; kept = (double)N2 / (double)N1 (0 when N1 = 0) is written into that model, which is the fit's result.  One call, at
 *   most max_frames frames; nothing accumulates across calls.
 * SOLVE (vp_keymatte_solve_host, and the same source in one device lane).  With S.. the moments and N = S11 (index 20):
 *   N < 1: every number of the model is 0 except inv00 = inv11 = inv22 = 1 / (sigma_min * sigma_min), kept = 1 and status = 1.  Otherwise
 *   Nd = (double)N; the means mx = (double)Sx / Nd, my, mR, mG, mB alike; the centred second moments
 *   Cab = (double)(N * Sab - Sa * Sb) / (Nd * Nd) for ab in xx, xy, yy, xc, yc and the six cd (c, d channels, c <= d): the integer is
 *   exact (128 bits) and converted through its magnitude u = hi * 2^64 + lo as (double)hi * 2^64 + (double)lo, then given its sign, so a
 *   border of one colour has slopes and residuals of exactly 0.
 *   det = Cxx * Cyy - Cxy * Cxy.  degenerate = N < 16 or not (det > 1e-9 * (Cxx * Cyy)).
 *   Per channel c, not degenerate: px = (Cxc * Cyy - Cyc * Cxy) / det, py = (Cyc * Cxx - Cxc * Cxy) / det; degenerate: px = py = 0.
 *   p0 = (mc - px * mx) - py * my.  The plane is b_c(x, y) = (p0 + px * (double)x) + py * (double)y.
 *   Residual covariance, c <= d: Rcd = (Ccd - px_c * Cxd) - py_c * Cyd; a negative Rcc is replaced by 0.
 *   residual_rms = sqrt(((R00 + R11) + R22) / 3.0).
 *   Sigma = R + (sigma_min * sigma_min) I: a = S00, b = S01, c = S02, d = S11, e = S12, f = S22.  Adjugate: A00 = d * f - e * e,
 *   A01 = c * e - b * f, A02 = b * e - c * d, A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
 *   D = (a * A00 + b * A01) + c * A02; inv_ij = A_ij / D.  When not (D > 0): inv = I / (sigma_min * sigma_min) and status = 1
 *   (the planes stay).  Otherwise status = 1 when degenerate, else 0.  kept = 1.
 *   The model record, VP_KEYMATTE_MODEL_DOUBLES float64: [0..8] p0, px, py of R, of G, of B; [9..14] inv00 inv01 inv02 inv11 inv12
 *   inv22; [15] N; [16] kept; [17] residual_rms; [18] status.
 * APPLY, per pixel (x, y) with channels c0 c1 c2:
 *   r_c = (double)c - b_c(x, y);
 *   q0 = (inv00 * r0 + inv01 * r1) + inv02 * r2, q1 = (inv01 * r0 + inv11 * r1) + inv12 * r2, q2 = (inv02 * r0 + inv12 * r1) + inv22 * r2;
 *   d2 = (r0 * q0 + r1 * q1) + r2 * q2;
 *   t = min(max((d2 - lo * lo) / (hi * hi - lo * lo), 0), 1) (a NaN gives 0); a = (t * t) * (3.0 - 2.0 * t);
 *   raw key p = (uint8)floor(255.0 * a + 0.5).  No square root.
 *   radius = 0: the matte is p.  Otherwise the guide is I = (77 R + 150 G + 29 B + 128) >> 8, and with the (2 radius + 1)^2 window centred
 *   on the pixel and clipped to the image, n_w its pixel count, the integer sums sI, sp, sII = sum I^2, sIp = sum I p over it:
 *   a_k = (double)(sIp * n_w - sI * sp) / ((double)(sII * n_w - sI * sI) + eps * (double)(n_w * n_w));
 *   b_k = ((double)sp - a_k * (double)sI) / (double)n_w;
 *   sa, sb: the sums of a_k, b_k over the same clipped window: first per row the sum over its columns in increasing x, then the sum of
 *   those row sums in increasing y, each sum starting from +0.0;
 *   q = (sa / (double)n_w) * (double)I + sb / (double)n_w;   matte = (uint8)floor(min(max(q, 0), 255) + 0.5).
 * Defaults of the Python layer: trim 16, sigma_min 2 grey levels, lo 4 and hi 10 (standard deviations of the backdrop), radius 4,
 * eps 25 (grey levels squared).  They come from synthetic scenes and are UNTUNED on real footage.
 * A frame's matte depends on the model and that frame alone: the same bytes in any batch.  No floating-point atomics anywhere.
 * ---------------------------------------------------------------------------------------------- */
#define VP_KEYMATTE_MAX_FRAMES 4096
#define VP_KEYMATTE_MAX_SIZE 1024
#define VP_KEYMATTE_MAX_RADIUS 16
#define VP_KEYMATTE_MODEL_DOUBLES 19
typedef struct vp_keymatte_desc {
  uint32_t struct_bytes;  /* sizeof(vp_keymatte_desc) of the caller's build: must equal vp_keymatte_desc_size() */
  int32_t max_frames;     /* frames per call: 1 .. VP_KEYMATTE_MAX_FRAMES */
  int32_t max_height;     /* 16 .. VP_KEYMATTE_MAX_SIZE */
  int32_t max_width;      /* 16 .. VP_KEYMATTE_MAX_SIZE */
  int32_t max_radius;     /* 0 .. VP_KEYMATTE_MAX_RADIUS; 0 leaves the guided filter's planes out of the workspace */
} vp_keymatte_desc;
size_t vp_keymatte_desc_size(void);
typedef struct vp_keymatte vp_keymatte_t;
/* 0 on a refused descriptor (vp_last_error names the field).  With max_radius > 0 the workspace holds a_k and b_k as float64 planes:
 * 16 bytes per pixel of max_frames x max_height x max_width. */
size_t vp_keymatte_workspace_bytes(const vp_keymatte_desc* d);
/* Host only: touches no device memory.  workspace: DEVICE memory the caller keeps alive as long as the handle.  The model is undefined
 * until vp_keymatte_fit or vp_keymatte_set_model has run. */
int vp_keymatte_create(const vp_keymatte_desc* d, void* workspace, size_t workspace_bytes, vp_keymatte_t** out);
void vp_keymatte_destroy(vp_keymatte_t* h);
/* FIT on n = 1 .. max_frames frames (DEVICE).  Refused before anything is enqueued, vp_last_error naming the field: n, height, width,
 * row_pitch < 3 * width, frame_stride < (height - 1) * row_pitch + 3 * width, band, side_rows, trim not finite or < 0, sigma_min not
 * finite or <= 0.  One fill of the moments and four launches on `stream` (moments, solve, trimmed moments, solve); nothing is read back;
 * never waits, never allocates. */
int vp_keymatte_fit(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                    int band, int side_rows, double trim, double sigma_min, void* stream);
/* APPLY with the handle's model.  raw: NULL or DEVICE uint8 [n, height, width], the raw key p; matte: DEVICE uint8 [n, height, width].
 * Refused before anything is enqueued, vp_last_error naming the field: n, height, width, row_pitch, frame_stride as above; lo, hi not
 * finite or not 0 <= lo < hi; radius outside 0 .. max_radius; eps not finite or <= 0.  One launch at radius 0, else two (the
 * coefficients a_k, b_k of every pixel into the workspace; their window means and the matte); never waits, never allocates. */
int vp_keymatte_apply(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                      double lo, double hi, int radius, double eps, unsigned char* raw, unsigned char* matte, void* stream);
/* model: DEVICE float64 [VP_KEYMATTE_MODEL_DOUBLES] on an 8-byte boundary; one device-to-device copy enqueued on `stream`. */
int vp_keymatte_get_model(vp_keymatte_t* h, double* model, void* stream);
int vp_keymatte_set_model(vp_keymatte_t* h, const double* model, void* stream);
/* "moments": int64 [2, 21], pass 1 and pass 2 of the last fit; "model": float64 [VP_KEYMATTE_MODEL_DOUBLES] */
int vp_keymatte_tensor(vp_keymatte_t* h, const char* name, void** ptr, int64_t shape[4]);
/* Host only: SOLVE above, the source the device lane runs.  model: VP_KEYMATTE_MODEL_DOUBLES doubles.  VP_ERR_ARG on a null pointer or
 * a sigma_min that is not finite or <= 0. */
int vp_keymatte_solve_host(const int64_t moments[21], double sigma_min, double* model);

/* FOREGROUND: the subject's own colours on the matte's soft edge.  A frame pixel is I = a F + (1 - a) B; the training input frame x matte
 * and an enrolment photo x matte therefore carry a fringe of backdrop colour, which shows as a halo over any other background.  The
 * handle's model knows B (the planes b_c), so F is recovered per pixel and channel, float64 in the order written, no fused multiply-add:
 *   m = 0: out = 0.  m = 255: e_c = (double)I_c.  Otherwise e_c = b_c(x, y) + ((double)I_c - b_c(x, y)) * (255.0 / (double)m), then
 *   e_c = min(max(e_c, 0), 255).
 *   Despill: v_c = b_c(W / 2, H / 2) (integer divisions); the key channel k is the largest v_c, the lowest index on a tie; i < j the other
 *   two; lead = v_k - max(v_i, v_j).  When lead >= 16 and despill > 0: e_k = e_k - despill * max(0, e_k - (e_i + e_j) / 2.0).  (A neutral
 *   backdrop has no spill to remove.)
 *   out_c = (uint8)floor(e_c + 0.5).
 * It is exact where the matte is: with KeyMatte's own matte it roughly halves the edge's colour error, no more.
 * frames as in vp_keymatte_apply; matte and out contiguous: DEVICE uint8 [n, height, width] and [n, height, width, 3].  Refused before
 * anything is enqueued, vp_last_error naming the field: n, height, width, row_pitch, frame_stride, matte, out, despill not in 0 .. 1.
 * One launch, no workspace; never waits, never allocates.  The call returns no word on which despill case held: the model is on the
 * device and nothing is read back.  The answer is a host read of the model's planes at the centre (KeyMatte.spill in the Python layer),
 * by the rule above.  (Not named vp_keymatte_*: that family's list is closed.) */
int vp_key_foreground(vp_keymatte_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                      const unsigned char* matte, double despill, unsigned char* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clean-up of an alpha matte, on the device: the stage every keyer puts behind its key.  A key marks everything that is not backdrop as
 * subject (noise speckle, a prop, the frame's edge where the backdrop ends) and a patch of backdrop colour on the subject as a hole.
 * Works on any uint8 matte (vp_keymatte_apply's, or one from a file).  It is component bookkeeping, not a matting solve: it moves no
 * edge and knows nothing of colour.  csrc/matte_clean.hip; the union-find core is csrc/matte_clean_core.h.
 *
 * Per frame, integers only, 16 <= height, width <= 1024; pixel (x, y) has the index y * W + x:
 * COMPONENTS.  S = {m >= support}, split into 8-connected components.  A component's label is the smallest index among its pixels
 *   (so labels depend on no schedule).  Per component: area, its pixel count; bottom: it has a pixel in row H - 1 (the torso leaves
 *   through the bottom); anchored: it holds one of the frame's k anchor pixels (x, y) (anchors outside the frame are ignored).
 *   pass = area >= min_area and (keep == ALL or bottom or anchored).  When keep == ANCHORED, the frame has components and none
 *   passes, all of them are kept and status bit 1 is set (an untouched matte is better than an empty one); otherwise the kept ones are
 *   those that pass.
 *   m1 = m on a pixel of a kept component, 0 on a pixel of a removed one.  A pixel with m < support keeps its value when a pixel of a
 *   kept component lies within Chebyshev distance `grow` of it (the kept component's soft fringe) and becomes 0 elsewhere (the haze).
 * HOLES (skipped when max_hole = 0).  N = {m1 < core}, split into 4-connected components.  A component of N that has no pixel on any of
 *   the four frame edges and at most max_hole pixels becomes 255, its soft rim included.
 * REPORT, int32 [8] per frame: components of S; kept; pixels of removed components; pixels with 0 < m < support that became 0; holes
 *   filled; pixels filled; status (bit 1: nothing passed, all kept - then kept = components; bit 2: a step cap of the labelling was
 *   reached, which a correct run cannot: the result is then not to be used); 0.
 * min_area = -1 means H * W / 1024, max_hole = -1 means H * W / 256; the Python layer's other defaults are support 32, core 224,
 * grow 4, keep ANCHORED.  All of them are UNTUNED on real footage.
 * A frame's result depends on that frame and its anchors alone: the same bytes in any batch.  No floating-point anything; integer
 * atomics only; no launch waits on another workgroup.
 * ---------------------------------------------------------------------------------------------- */
#define VP_MATTECLEAN_MAX_FRAMES 4096
#define VP_MATTECLEAN_MAX_SIZE 1024
#define VP_MATTECLEAN_MAX_GROW 16
#define VP_MATTECLEAN_MAX_ANCHORS 256
#define VP_MATTECLEAN_REPORT_INTS 8
#define VP_MATTECLEAN_KEEP_ALL 0
#define VP_MATTECLEAN_KEEP_ANCHORED 1
typedef struct vp_matteclean_desc {
  uint32_t struct_bytes;  /* sizeof(vp_matteclean_desc) of the caller's build: must equal vp_matteclean_desc_size() */
  int32_t max_frames;     /* frames per call: 1 .. VP_MATTECLEAN_MAX_FRAMES */
  int32_t max_height;     /* 16 .. VP_MATTECLEAN_MAX_SIZE */
  int32_t max_width;      /* 16 .. VP_MATTECLEAN_MAX_SIZE */
} vp_matteclean_desc;
size_t vp_matteclean_desc_size(void);
typedef struct vp_matteclean vp_matteclean_t;
/* 0 on a refused descriptor (vp_last_error names the field).  At most 12 bytes per pixel of max_frames x max_height x max_width plus
 * 4096: the labels (4), the hole pass's parents (4), one record per pixel pair (2) and the report. */
size_t vp_matteclean_workspace_bytes(const vp_matteclean_desc* d);
/* Host only: touches no device memory.  workspace: DEVICE memory the caller keeps alive as long as the handle. */
int vp_matteclean_create(const vp_matteclean_desc* d, void* workspace, size_t workspace_bytes, vp_matteclean_t** out);
void vp_matteclean_destroy(vp_matteclean_t* h);
/* matte, out: DEVICE uint8 [n, height, width], contiguous; out is the matte itself or disjoint from it (an overlap is refused); anchors: NULL with k = 0, else DEVICE int32
 * [n, k, 2] of (x, y).  Refused before anything is enqueued, vp_last_error naming the field: n, height, width, support and core outside
 * 1 .. 255, min_area and max_hole outside -1 .. height * width, grow outside 0 .. 16, keep, k outside 0 .. 256, anchors, out.  One fill of
 * the report and twelve launches on `stream` (seven with max_hole = 0); nothing is read back; never waits, never allocates. */
int vp_matteclean_clean(vp_matteclean_t* h, const unsigned char* matte, int n, int height, int width, int support, int core, int min_area,
                        int max_hole, int grow, int keep, const int* anchors, int k, unsigned char* out, void* stream);
/* "labels": int32 [max_frames, height, width] of the last call (the descriptor's before the first): -1 outside S, else the component's
 * label; "report": int32 [max_frames, VP_MATTECLEAN_REPORT_INTS] */
int vp_matteclean_tensor(vp_matteclean_t* h, const char* name, void** ptr, int64_t shape[4]);

/* ------------------------------------------------------------------------------------------------
 * Trimap and closed-form matting solve, on the device: stages two and three of the matte that step 6 of the reference's
 * datasets/make_data_from_GRID.py makes (:654-659 the trimap from a 30 x 30 erosion and a 20 x 20 dilation of the segmentation mask,
 * :670-672 the matting network's alpha with the known pixels forced afterwards).  In place of the matting network: the closed-form
 * matting of Levin, Lischinski and Weiss (the matting Laplacian, applied by window sums as in He, Sun and Tang's large-kernel form),
 * a float64 linear solve inside the trimap's unknown band.  It needs no weights and no backdrop model: any binary mask will do.
 * csrc/matte_solve.hip; tests/matte_solve_ref.py restates every number below in numpy.
 *
 * 16 <= height, width <= 1024; frames are addressed as in vp_keymatte_apply (row_pitch, frame_stride, RGB bytes I_c, c = 0 1 2).
 * TRIMAP, integers only.  A k x k square covers the offsets d = -(k / 2) .. k - 1 - (k / 2) (integer division) on each axis; the square
 *   at (x, y) is the pixels (x + dx, y + dy) of it that lie inside the image (pixels outside the image neither erode nor dilate).
 *   fg(x, y): every pixel of the erode x erode square at (x, y) has m >= core.  maybe(x, y): some pixel of the dilate x dilate square at
 *   (x, y) has m >= support.  trimap = 255 on fg, else 127 on maybe, else 0 (127 is what the reference's mask2 + mask // 2 gives).
 *   1 <= erode, dilate <= VP_MATTESOLVE_MAX_SQUARE; 0 means the default by frame size: the reference's 30 and 20 are for 720 x 576
 *   video, 1 / 19 and 1 / 29 of the shorter side, so erode = max(5, min(64, min(H, W) / 19)), dilate = max(5, min(64, min(H, W) / 29)).
 *   This is the definition, not a claim of equality with any library's erode and dilate.
 *   The call also writes, per 32 x 32 tile (the solver's tiling, tiles in row-major order), whether the tile holds a pixel of value 127:
 *   tensor "tiles".  The solve takes any trimap, so it forms these flags again from the trimap it is given.
 * SOLVE.  A trimap pixel is known 0 (value 0), known 1 (value 255) or unknown (anything else); U the unknown pixels; k = 1 on known-1
 *   pixels and 0 elsewhere.  radius r in 1 .. max_radius; w_j the (2 r + 1)^2 window centred on j clipped to the image, n_j its pixel
 *   count.  All float64, in the order written, no fused multiply-add; every window sum takes its rows in increasing y and within a row
 *   increasing x, starting from +0.0.
 *   MOMENTS of w_j, from exact integer sums S_c = sum I_c, S_cd = sum I_c I_d (c <= d): nd = (double)n_j;
 *   mu_c = (double)S_c / nd;  Sigma_cd = (double)(n_j * S_cd - S_c * S_d) / (nd * nd);  M = Sigma + (eps / nd) Id with
 *   a = M00, b = M01, c = M02, d = M11, e = M12, f = M22;  adjugate A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d,
 *   A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;  D = (a * A00 + b * A01) + c * A02;  Inv_cd = A_cd / D.
 *   LAPLACIAN of a plane p: per window j  mp = (sum p) / nd,  v_c = (sum (double)I_c * p) / nd - mu_c * mp,
 *   a_j = Inv v (row c: (Inv_c0 * v0 + Inv_c1 * v1) + Inv_c2 * v2),  b_j = mp - ((a_j0 * mu_0 + a_j1 * mu_1) + a_j2 * mu_2);
 *   per pixel i with sa_c, sb the sums of a_jc, b_j over the windows j in w_i (the windows that hold i):
 *   (L p)_i = (double)n_i * p_i - (((sa_0 * I_i0 + sa_1 * I_i1) + sa_2 * I_i2) + sb).
 *   DIAGONAL: diag_i = sum over j in w_i of 1 - (1 + ((d_0 * q_0 + d_1 * q_1) + d_2 * q_2)) / (double)n_j with d = I_i - mu_j and q = Inv_j d.
 *   SYSTEM: L_UU x = b, b = -(L k)_U, by conjugate gradients preconditioned with 1 / diag_i, from x = 0: r = b, z = r / diag (as
 *   (1 / diag) * r), p = z.  Iteration it = 0, 1, ..: the frame stops when r.r <= tol * tol * b.b (then iterations = it); otherwise
 *   q = (L p)_U with p = 0 outside U; a frame whose p.q is not positive or not finite stops where it is with status bit 2; alpha = r.z /
 *   p.q; x += alpha p; r -= alpha q; z = r / diag; beta = (new r.z) / (old r.z); p = z + beta p.  After `iters` iterations the frame
 *   stops with iterations = iters.  b.b = 0 (no constraint reaches the band, or the trimap has no unknown pixel): x = 0, zero
 *   iterations, status bit 1.
 *   Dot products: per 32 x 32 tile a fixed tree over the workgroup's lanes, then the tiles of the frame in a fixed order, summed again
 *   by every workgroup that needs the scalar.  No floating-point atomics.  A frame's float64 solution, iteration count and matte are
 *   therefore the same bits in any batch, at any batch position and on every run.
 *   Matte: 0 or 255 on the known pixels (the reference's :671-672), (uint8)floor(min(max(x, 0), 1) * 255.0 + 0.5) on U.
 *   Schedule: two fills, one init launch, two launches per iteration for all `iters` iterations (the host never learns that a frame
 *   stopped: a stopped frame's workgroups and the tiles without an unknown pixel return at once), one finish launch.  No launch waits
 *   on another workgroup.
 * REPORT, per frame VP_MATTESOLVE_REPORT_INTS int32 (32 bytes): [0] unknown pixels, [1] iterations, [2] status, [3] 0, then at byte 16
 *   the final relative residual sqrt(r.r / b.b) of the recurrence as one float64 (0 with status bit 1), [6] [7] 0.
 * Defaults of the Python layer: support 32, core 224, erode and dilate by the rule above, radius 1, eps 1 (grey levels squared),
 * iters 512, tol 1e-6.  They come from synthetic scenes (DESIGN.md 6 has the grid) and are UNTUNED on real footage.
 * ---------------------------------------------------------------------------------------------- */
#define VP_MATTESOLVE_MAX_FRAMES 4096
#define VP_MATTESOLVE_MAX_SIZE 1024
#define VP_MATTESOLVE_MAX_RADIUS 3
#define VP_MATTESOLVE_MAX_SQUARE 64
#define VP_MATTESOLVE_MAX_ITERS 1024
#define VP_MATTESOLVE_REPORT_INTS 8
typedef struct vp_mattesolve_desc {
  uint32_t struct_bytes;  /* sizeof(vp_mattesolve_desc) of the caller's build: must equal vp_mattesolve_desc_size() */
  int32_t max_frames;     /* frames per call: 1 .. VP_MATTESOLVE_MAX_FRAMES */
  int32_t max_height;     /* 16 .. VP_MATTESOLVE_MAX_SIZE */
  int32_t max_width;      /* 16 .. VP_MATTESOLVE_MAX_SIZE */
  int32_t max_radius;     /* 1 .. VP_MATTESOLVE_MAX_RADIUS */
} vp_mattesolve_desc;
size_t vp_mattesolve_desc_size(void);
typedef struct vp_mattesolve vp_mattesolve_t;
/* 0 on a refused descriptor (vp_last_error names the field).  48 bytes per pixel of max_frames x max_height x max_width (six float64
 * planes: x, r, 1 / diag, two of p, L p) plus 44 bytes per 32 x 32 tile (five partial sums and the tile's flag), 36 per frame and at
 * most 4096. */
size_t vp_mattesolve_workspace_bytes(const vp_mattesolve_desc* d);
/* Host only: touches no device memory.  workspace: DEVICE memory the caller keeps alive as long as the handle. */
int vp_mattesolve_create(const vp_mattesolve_desc* d, void* workspace, size_t workspace_bytes, vp_mattesolve_t** out);
void vp_mattesolve_destroy(vp_mattesolve_t* h);
/* TRIMAP.  matte, out: DEVICE uint8 [n, height, width], contiguous and disjoint (an overlap is refused).  Refused before anything is
 * enqueued, vp_last_error naming the field: n, height, width, support and core outside 1 .. 255, erode and dilate outside 0 .. 64, out.
 * One launch on `stream`; nothing is read back; never waits, never allocates. */
int vp_mattesolve_trimap(vp_mattesolve_t* h, const unsigned char* matte, int n, int height, int width, int support, int core, int erode,
                         int dilate, unsigned char* out, void* stream);
/* SOLVE.  trimap, matte: DEVICE uint8 [n, height, width], contiguous; matte is the trimap itself or disjoint from it (an overlap at
 * another address is refused).  Refused before anything is
 * enqueued, vp_last_error naming the field: n, height, width, row_pitch, frame_stride (as vp_keymatte_apply), radius outside
 * 1 .. max_radius, eps not finite or <= 0, trimap, iters outside 1 .. VP_MATTESOLVE_MAX_ITERS, tol not finite or < 0, matte.
 * 2 fills and 2 * iters + 2 launches on `stream`; nothing is read back; never waits, never allocates. */
int vp_mattesolve_solve(vp_mattesolve_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                        const unsigned char* trimap, int radius, double eps, int iters, double tol, unsigned char* matte, void* stream);
/* The single op behind the solve, for parity tests: out = L p for DEVICE float64 planes [n, height, width] on 8-byte boundaries,
 * contiguous and disjoint, no masking.  Refusals as above (frames, radius, eps, p, out).  One launch; touches no workspace. */
int vp_mattesolve_laplacian(vp_mattesolve_t* h, const unsigned char* frames, size_t row_pitch, size_t frame_stride, int n, int height, int width,
                            int radius, double eps, const double* p, double* out, void* stream);
/* "alpha": float64 [max_frames, height, width] of the last SOLVE (the descriptor's before the first; a trimap call of another size does
 * not change it): the unclamped solution on U, k on the known pixels; "report": int32 [max_frames, VP_MATTESOLVE_REPORT_INTS]; "tiles": int32 [max_frames, ceil(height / 32),
 * ceil(width / 32)] with the height and width of the last trimap or solve, whichever came later: 1 where the tile holds an unknown pixel */
int vp_mattesolve_tensor(vp_mattesolve_t* h, const char* name, void** ptr, int64_t shape[4]);

/* Host helper: CRC-32C (Castagnoli, the checksum of TensorFlow checkpoint bundles) of `n` bytes, continuing from `crc` (0 to start). */
unsigned vp_crc32c(const void* data, size_t n, unsigned crc);

#ifdef __cplusplus
}
#endif
#endif /* VP_HIP_H_ */
