"""ctypes binding of libvp_hip.so (include/vp_hip.h).  Fails loudly when the library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VP_LIB", os.path.join(_HERE, "libvp_hip.so"))   # VP_LIB: ablation builds only

VP_F32, VP_BF16 = 0, 1
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
BN_PATH_PLANNER, BN_PATH_TWO_PASS, BN_PATH_ONE_LAUNCH = 0, 1, 2      # include/vp_hip.h VP_BN_PATH_*


class PixReferDesc(ctypes.Structure):
  _fields_ = [("batch", ctypes.c_int), ("height", ctypes.c_int), ("ngf", ctypes.c_int), ("ndf", ctypes.c_int),
              ("dtype", ctypes.c_int), ("training", ctypes.c_int), ("l1_weight", ctypes.c_float),
              ("gan_weight", ctypes.c_float), ("per_sample_bn", ctypes.c_int),
              # schedule of a training plan (0 = default; include/vp_hip.h)
              ("streams", ctypes.c_int), ("d_backward_fork", ctypes.c_int), ("d_beside_vgg", ctypes.c_int)]


class ConvDesc(ctypes.Structure):
  _fields_ = [("kind", ctypes.c_int), ("n", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int),
              ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("ksize", ctypes.c_int), ("stride", ctypes.c_int),
              ("pad", ctypes.c_int), ("dtype", ctypes.c_int), ("in_act", ctypes.c_int), ("out_act", ctypes.c_int)]


class LogMelDesc(ctypes.Structure):
  _fields_ = [("sample_rate", ctypes.c_int), ("num_mel_bins", ctypes.c_int), ("win_length", ctypes.c_int),
              ("hop_step", ctypes.c_int), ("fft_length", ctypes.c_int), ("lower_hz", ctypes.c_float),
              ("upper_hz", ctypes.c_float), ("batch", ctypes.c_int), ("samples", ctypes.c_int)]


class BfmNetDesc(ctypes.Structure):
  _fields_ = [("batch", ctypes.c_int), ("frames", ctypes.c_int), ("num_mel_bins", ctypes.c_int), ("trunk_dtype", ctypes.c_int)]


class BfmStreamDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_int), ("max_chunk_frames", ctypes.c_int), ("num_mel_bins", ctypes.c_int),
              ("trunk_dtype", ctypes.c_int), ("sample_rate", ctypes.c_int), ("lower_hz", ctypes.c_float), ("upper_hz", ctypes.c_float)]


class BfmStreamGroupDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_int), ("slots", ctypes.c_int), ("max_chunk_frames", ctypes.c_int), ("num_mel_bins", ctypes.c_int),
              ("trunk_dtype", ctypes.c_int), ("sample_rate", ctypes.c_int), ("lower_hz", ctypes.c_float), ("upper_hz", ctypes.c_float)]


BFMSTREAM_GROUP_MAX_SLOTS = 128      # include/vp_hip.h VP_BFMSTREAM_GROUP_MAX_SLOTS


class PuppetDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_int), ("slots", ctypes.c_int), ("frame_batch", ctypes.c_int), ("img_size", ctypes.c_int),
              ("face_size", ctypes.c_int)]


PUPPET_MAX_SLOTS = 128               # include/vp_hip.h VP_PUPPET_MAX_SLOTS


class JpegDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
              ("quality", ctypes.c_int32)]


class PngDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
              ("channels", ctypes.c_int32), ("filter", ctypes.c_int32)]


PNG_U8, PNG_F32 = 0, 1               # include/vp_hip.h vp_png_dtype


class JpegDecDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_files", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_width", ctypes.c_int32),
              ("max_file_bytes", ctypes.c_int32), ("max_segments_per_file", ctypes.c_int32), ("bgr", ctypes.c_int32)]


class JpegDecFile(ctypes.Structure):
  _fields_ = [("meta_offset", ctypes.c_uint64), ("file_offset", ctypes.c_uint64), ("file_bytes", ctypes.c_int32), ("width", ctypes.c_int32),
              ("height", ctypes.c_int32), ("sampling", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("n_segments", ctypes.c_int32),
              ("tq", ctypes.c_uint8 * 3), ("td", ctypes.c_uint8 * 3), ("ta", ctypes.c_uint8 * 3), ("reserved", ctypes.c_uint8 * 3)]


JPEGDEC_META_BYTES = 6336            # include/vp_hip.h VP_JPEGDEC_META_BYTES


class PcmInDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_int), ("slots", ctypes.c_int), ("out_rate", ctypes.c_int), ("max_in_frames", ctypes.c_int),
              ("n_rates", ctypes.c_int), ("rates", ctypes.c_int * 8)]


PCMIN_MAX_SLOTS, PCMIN_MAX_CHANNELS = 128, 8      # include/vp_hip.h VP_PCMIN_MAX_SLOTS, VP_PCMIN_MAX_CHANNELS
PCM_S16, PCM_F32 = 0, 1


class FrameMetricsDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_width", ctypes.c_int32)]


FRAME_METRICS_MAX_FRAMES = 4096      # include/vp_hip.h VP_FRAME_METRICS_MAX_FRAMES


class AviMuxDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("row_bytes", ctypes.c_int32), ("slots", ctypes.c_int32),
              ("max_samples", ctypes.c_int32)]


AVIMUX_MAX_FRAMES, AVIMUX_MAX_SLOTS = 4096, 128   # include/vp_hip.h VP_AVIMUX_MAX_FRAMES, VP_AVIMUX_MAX_SLOTS


class KeyMatteDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_width", ctypes.c_int32),
              ("max_radius", ctypes.c_int32)]


# include/vp_hip.h VP_KEYMATTE_MAX_FRAMES, VP_KEYMATTE_MAX_SIZE, VP_KEYMATTE_MAX_RADIUS, VP_KEYMATTE_MODEL_DOUBLES
KEYMATTE_MAX_FRAMES, KEYMATTE_MAX_SIZE, KEYMATTE_MAX_RADIUS, KEYMATTE_MODEL_DOUBLES = 4096, 1024, 16, 19


class MatteCleanDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_width", ctypes.c_int32)]


# include/vp_hip.h VP_MATTECLEAN_MAX_FRAMES, _MAX_SIZE, _MAX_GROW, _MAX_ANCHORS, _REPORT_INTS, _KEEP_ALL, _KEEP_ANCHORED
MATTECLEAN_MAX_FRAMES, MATTECLEAN_MAX_SIZE, MATTECLEAN_MAX_GROW, MATTECLEAN_MAX_ANCHORS, MATTECLEAN_REPORT_INTS = 4096, 1024, 16, 256, 8
MATTECLEAN_KEEP_ALL, MATTECLEAN_KEEP_ANCHORED = 0, 1


class MatteSolveDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_width", ctypes.c_int32),
              ("max_radius", ctypes.c_int32)]


# include/vp_hip.h VP_MATTESOLVE_MAX_FRAMES, _MAX_SIZE, _MAX_RADIUS, _MAX_SQUARE, _MAX_ITERS, _REPORT_INTS
MATTESOLVE_MAX_FRAMES, MATTESOLVE_MAX_SIZE, MATTESOLVE_MAX_RADIUS, MATTESOLVE_MAX_SQUARE, MATTESOLVE_MAX_ITERS, MATTESOLVE_REPORT_INTS = 4096, 1024, 3, 64, 1024, 8


class TriptychDesc(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_frames", ctypes.c_int32), ("size", ctypes.c_int32), ("face_size", ctypes.c_int32),
              ("max_side", ctypes.c_int32)]


TRIPTYCH_MAX_FRAMES, TRIPTYCH_MAX_SIZE = 4096, 1024   # include/vp_hip.h VP_TRIPTYCH_MAX_FRAMES, VP_TRIPTYCH_MAX_SIZE


class BfmObserveOpts(ctypes.Structure):
  _fields_ = [("struct_bytes", ctypes.c_uint32), ("visibility", ctypes.c_int32), ("raster_scale", ctypes.c_int32), ("prefilter", ctypes.c_int32),
              ("depth_tol", ctypes.c_float)]


class BfmModel(ctypes.Structure):
  _fields_ = [("nver", ctypes.c_int), ("ntri", ctypes.c_int), ("meanshape", ctypes.c_void_p), ("idBase", ctypes.c_void_p),
              ("exBase", ctypes.c_void_p), ("meantex", ctypes.c_void_p), ("texBase", ctypes.c_void_p), ("tri", ctypes.c_void_p),
              ("point_buf", ctypes.c_void_p), ("center", ctypes.c_double * 3), ("focal", ctypes.c_double),
              ("image_center", ctypes.c_double), ("sh", ctypes.c_double * 5)]


_P = ctypes.c_void_p
_SIGNATURES = {
    "vp_version": (ctypes.c_int, []),
    "vp_last_error": (ctypes.c_char_p, []),
    "vp_pixrefer_param_count": (ctypes.c_size_t, [ctypes.POINTER(PixReferDesc), ctypes.c_int]),
    "vp_pixrefer_param_info": (ctypes.c_int, [ctypes.POINTER(PixReferDesc), ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                              ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(ctypes.c_int64)]),
    "vp_pixrefer_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(PixReferDesc)]),
    "vp_pixrefer_validate_plan": (ctypes.c_int, [ctypes.POINTER(PixReferDesc)]),
    "vp_pixrefer_create": (ctypes.c_int, [ctypes.POINTER(PixReferDesc), _P, ctypes.c_size_t, _P, _P, _P, _P, _P, _P,
                                          ctypes.POINTER(_P)]),
    "vp_pixrefer_destroy": (None, [_P]),
    "vp_pixrefer_params_changed": (ctypes.c_int, [_P]),
    "vp_pixrefer_optimizer_stepped": (ctypes.c_int, [_P]),
    "vp_pixrefer_forward": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "vp_pixrefer_forward_fg3": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "vp_pixrefer_desc_size": (ctypes.c_size_t, []),
    "vp_pixrefer_backward": (ctypes.c_int, [_P, _P]),
    "vp_pixrefer_backward_update": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                   ctypes.c_float, ctypes.c_float, _P]),
    "vp_pixrefer_backward_d": (ctypes.c_int, [_P, _P]),
    "vp_pixrefer_backward_g": (ctypes.c_int, [_P, _P]),
    "vp_pixrefer_backward_d_fork": (ctypes.c_int, [_P, _P]),
    "vp_pixrefer_backward_d_join": (ctypes.c_int, [_P, _P]),
    "vp_pixrefer_backward_g_stages": (ctypes.c_int, []),
    "vp_pixrefer_backward_g_stage": (ctypes.c_int, [_P, ctypes.c_int, _P]),
    "vp_pixrefer_side_stream": (ctypes.c_void_p, [_P]),
    "vp_pixrefer_use_streams": (ctypes.c_int, [_P, ctypes.c_int]),
    "vp_pixrefer_set_option": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int]),
    "vp_pixrefer_fetch": (ctypes.c_int, [_P, ctypes.c_int, _P, _P]),
    "vp_pixrefer_counter": (ctypes.c_longlong, [_P, ctypes.c_char_p]),
    "vp_crc32c": (ctypes.c_uint, [_P, ctypes.c_size_t, ctypes.c_uint]),
    "vp_pixrefer_phase_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
    "vp_grad_pack_bf16": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P]),
    "vp_grad_unpack_bf16": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_float, _P]),
    "vp_pixrefer_update_bucket": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                 ctypes.c_float, _P]),
    "vp_resize_paste_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "vp_resize_paste_u8": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_resize_linear_table": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]),
    "vp_mm_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_mm_fwd_f32": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_mm_bwd_data_f32": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, _P, _P]),
    "vp_mm_bwd_weight_f32": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_mm_packed_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_mm_pack_desc_bytes": (ctypes.c_size_t, []),
    "vp_mm_pack_desc": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, _P]),
    "vp_mm_pack_table": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P]),
    "vp_mm_fwd_f32_packed": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_mm_bwd_data_f32_packed": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_pixrefer_mark_ms": (ctypes.c_float, [_P, ctypes.c_int, ctypes.c_int]),
    "vp_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "vp_tune": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "vp_reserve_streams": (ctypes.c_int, []),
    "vp_host_stream": (ctypes.c_void_p, []),
    "vp_pixrefer_pack_frames": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P]),
    "vp_profile_collect": (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    "vp_pixrefer_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int)]),
    "vp_adam_tf": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_float, ctypes.c_float, _P]),
    "vp_conv_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ConvDesc)]),
    "vp_conv_fwd": (ctypes.c_int, [ctypes.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "vp_conv_bwd_data": (ctypes.c_int, [ctypes.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "vp_conv_bwd_weight": (ctypes.c_int, [ctypes.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P]),
    "vp_conv3x3_c64_bwd_data_pooled_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ConvDesc)]),
    "vp_conv3x3_c64_bwd_data_pooled": (ctypes.c_int, [ctypes.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, ctypes.c_int, _P]),
    "vp_bn_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_bn_stats": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_float, _P, _P, _P, _P, _P, _P]),
    "vp_logmel_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(LogMelDesc)]),
    "vp_logmel_frames": (ctypes.c_int, [ctypes.POINTER(LogMelDesc)]),
    "vp_logmel_create": (ctypes.c_int, [ctypes.POINTER(LogMelDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_logmel_destroy": (None, [_P]),
    "vp_logmel_forward": (ctypes.c_int, [_P, _P, _P, _P]),
    "vp_bfmnet_param_count": (ctypes.c_size_t, []),
    "vp_bfmnet_param_info": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t),
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)]),
    "vp_bfmnet_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(BfmNetDesc)]),
    "vp_bfmnet_create": (ctypes.c_int, [ctypes.POINTER(BfmNetDesc), _P, ctypes.c_size_t, _P, _P, ctypes.POINTER(_P)]),
    "vp_bfmnet_destroy": (None, [_P]),
    "vp_bfmnet_params_changed": (ctypes.c_int, [_P]),
    "vp_bfmnet_forward": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "vp_bfmnet_set_decoder_dropout": (ctypes.c_int, [_P, _P, _P]),
    "vp_bfmnet_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_bfmstream_desc_size": (ctypes.c_size_t, []),
    "vp_bfmstream_context": (ctypes.c_int, [ctypes.POINTER(BfmStreamDesc)] + [ctypes.POINTER(ctypes.c_int)] * 5),
    "vp_bfmstream_frames_after": (ctypes.c_longlong, [ctypes.POINTER(BfmStreamDesc), ctypes.c_longlong, ctypes.c_int]),
    "vp_bfmstream_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(BfmStreamDesc)]),
    "vp_bfmstream_create": (ctypes.c_int, [ctypes.POINTER(BfmStreamDesc), _P, ctypes.c_size_t, _P, _P, ctypes.POINTER(_P)]),
    "vp_bfmstream_destroy": (None, [_P]),
    "vp_bfmstream_params_changed": (ctypes.c_int, [_P]),
    "vp_bfmstream_reset": (ctypes.c_int, [_P, _P]),
    "vp_bfmstream_ready": (ctypes.c_int, [_P, ctypes.c_longlong]),
    "vp_bfmstream_ready_finish": (ctypes.c_int, [_P]),
    "vp_bfmstream_push": (ctypes.c_int, [_P, _P, ctypes.c_longlong, _P, _P, _P]),
    "vp_bfmstream_finish": (ctypes.c_int, [_P, _P, _P, _P]),
    "vp_bfmstream_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_bfmstream_group_desc_size": (ctypes.c_size_t, []),
    "vp_puppet_desc_size": (ctypes.c_size_t, []),
    "vp_puppet_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(PuppetDesc)]),
    "vp_puppet_create": (ctypes.c_int, [ctypes.POINTER(PuppetDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_puppet_destroy": (None, [_P]),
    "vp_puppet_attach": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_puppet_set_backgrounds": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "vp_puppet_splice": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, _P, _P]),
    "vp_puppet_condition": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, _P, _P, _P, _P]),
    "vp_puppet_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_puppet_slot_info": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "vp_jpeg_desc_size": (ctypes.c_size_t, []),
    "vp_jpeg_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(JpegDesc)]),
    "vp_jpeg_frame_capacity": (ctypes.c_size_t, [ctypes.POINTER(JpegDesc)]),
    "vp_jpeg_create": (ctypes.c_int, [ctypes.POINTER(JpegDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_jpeg_encode": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_size_t, _P, _P]),
    "vp_jpeg_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_jpeg_header": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "vp_jpeg_destroy": (None, [_P]),
    "vp_png_desc_size": (ctypes.c_size_t, []),
    "vp_png_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(PngDesc)]),
    "vp_png_frame_capacity": (ctypes.c_size_t, [ctypes.POINTER(PngDesc)]),
    "vp_png_rows_per_strip": (ctypes.c_int, [ctypes.POINTER(PngDesc)]),
    "vp_png_create": (ctypes.c_int, [ctypes.POINTER(PngDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_png_encode": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_size_t, _P, _P]),
    "vp_png_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_png_header": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "vp_png_destroy": (None, [_P]),
    "vp_jpegdec_desc_size": (ctypes.c_size_t, []),
    "vp_jpegdec_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(JpegDecDesc)]),
    "vp_jpegdec_create": (ctypes.c_int, [ctypes.POINTER(JpegDecDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_jpegdec_destroy": (None, [_P]),
    "vp_jpegdec_decode": (ctypes.c_int, [_P, _P, ctypes.POINTER(JpegDecFile), ctypes.c_int, _P, ctypes.c_size_t, ctypes.c_size_t, _P, _P]),
    "vp_jpegdec_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_jpegdec_scan_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(JpegDecDesc), ctypes.c_int]),
    "vp_jpegdec_enable_scan": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]),
    "vp_pcmin_desc_size": (ctypes.c_size_t, []),
    "vp_pcmin_ratio": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "vp_pcmin_bank": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _P]),
    "vp_pcmin_samples_after": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int]),
    "vp_pcmin_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(PcmInDesc)]),
    "vp_pcmin_create": (ctypes.c_int, [ctypes.POINTER(PcmInDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_pcmin_destroy": (None, [_P]),
    "vp_pcmin_open_slot": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_pcmin_ready": (ctypes.c_longlong, [_P, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    "vp_pcmin_push": (ctypes.c_int, [_P, _P, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int), _P, _P]),
    "vp_frame_metrics_desc_size": (ctypes.c_size_t, []),
    "vp_frame_metrics_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(FrameMetricsDesc)]),
    "vp_frame_metrics_create": (ctypes.c_int, [ctypes.POINTER(FrameMetricsDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_frame_metrics_destroy": (None, [_P]),
    "vp_frame_metrics_u8": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, _P, _P]),
    "vp_frame_metrics_f32": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_double, ctypes.c_double, _P, _P]),
    "vp_frame_metrics_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_avimux_desc_size": (ctypes.c_size_t, []),
    "vp_avimux_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(AviMuxDesc)]),
    "vp_avimux_out_capacity": (ctypes.c_size_t, [ctypes.POINTER(AviMuxDesc)]),
    "vp_avimux_table_bytes": (ctypes.c_size_t, [ctypes.POINTER(AviMuxDesc), ctypes.c_int]),
    "vp_avimux_create": (ctypes.c_int, [ctypes.POINTER(AviMuxDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_avimux_segment": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P, ctypes.c_int, _P, _P, _P, ctypes.c_int, _P, ctypes.c_size_t, _P]),
    "vp_avimux_destroy": (None, [_P]),
    "vp_triptych_desc_size": (ctypes.c_size_t, []),
    "vp_triptych_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(TriptychDesc)]),
    "vp_triptych_create": (ctypes.c_int, [ctypes.POINTER(TriptychDesc), _P, ctypes.c_size_t, _P, ctypes.POINTER(_P)]),
    "vp_triptych_build": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P]),
    "vp_triptych_mask": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P]),
    "vp_triptych_fill_holes": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_triptych_blur_taps": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "vp_triptych_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_triptych_destroy": (None, [_P]),
    "vp_keymatte_desc_size": (ctypes.c_size_t, []),
    "vp_keymatte_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(KeyMatteDesc)]),
    "vp_keymatte_create": (ctypes.c_int, [ctypes.POINTER(KeyMatteDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_keymatte_destroy": (None, [_P]),
    "vp_keymatte_fit": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_double, _P]),
    "vp_keymatte_apply": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_int, ctypes.c_double, _P, _P, _P]),
    "vp_keymatte_get_model": (ctypes.c_int, [_P, _P, _P]),
    "vp_keymatte_set_model": (ctypes.c_int, [_P, _P, _P]),
    "vp_keymatte_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_keymatte_solve_host": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "vp_key_foreground": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_double, _P, _P]),
    "vp_matteclean_desc_size": (ctypes.c_size_t, []),
    "vp_matteclean_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(MatteCleanDesc)]),
    "vp_matteclean_create": (ctypes.c_int, [ctypes.POINTER(MatteCleanDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_matteclean_destroy": (None, [_P]),
    "vp_matteclean_clean": (ctypes.c_int, [_P, _P] + [ctypes.c_int] * 9 + [_P, ctypes.c_int, _P, _P]),
    "vp_matteclean_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_mattesolve_desc_size": (ctypes.c_size_t, []),
    "vp_mattesolve_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(MatteSolveDesc)]),
    "vp_mattesolve_create": (ctypes.c_int, [ctypes.POINTER(MatteSolveDesc), _P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "vp_mattesolve_destroy": (None, [_P]),
    "vp_mattesolve_trimap": (ctypes.c_int, [_P, _P] + [ctypes.c_int] * 7 + [_P, _P]),
    "vp_mattesolve_solve": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_int, ctypes.c_double, _P, _P]),
    "vp_mattesolve_laplacian": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_double, _P, _P, _P]),
    "vp_mattesolve_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_bfm_reconstruct_rows": (ctypes.c_int, [ctypes.POINTER(BfmModel), _P, _P, ctypes.c_int, _P, ctypes.c_int, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_bfmstream_group_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(BfmStreamGroupDesc)]),
    "vp_bfmstream_group_plan_info": (ctypes.c_int, [ctypes.POINTER(BfmStreamGroupDesc), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "vp_bfmstream_group_create": (ctypes.c_int, [ctypes.POINTER(BfmStreamGroupDesc), _P, ctypes.c_size_t, _P, _P, ctypes.POINTER(_P)]),
    "vp_bfmstream_group_destroy": (None, [_P]),
    "vp_bfmstream_group_params_changed": (ctypes.c_int, [_P]),
    "vp_bfmstream_group_reset_slot": (ctypes.c_int, [_P, ctypes.c_int, _P]),
    "vp_bfmstream_group_ready": (ctypes.c_longlong, [_P, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "vp_bfmstream_group_push": (ctypes.c_int, [_P, _P, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int), _P, _P, _P]),
    "vp_bfmstream_group_tensor": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "vp_gru_seq_state": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_maxpool2x2_fwd": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_maxpool2x2_bwd": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_maxpool2x2_bwd_code": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_composite_fwd": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P]),
    "vp_gan_loss": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_float, ctypes.c_int, _P]),
    "vp_dwconv7x3_bn_act": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_dwconv7x3_bn_act_t": (ctypes.c_int, [_P, _P, _P, _P] + [ctypes.c_int] * 5 + [_P]),
    "vp_conv_first_fwd": (ctypes.c_int, [_P, _P, _P, _P] + [ctypes.c_int] * 4 + [_P]),
    "vp_dwproj_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "vp_dwproj_fwd": (ctypes.c_int, [_P] * 6 + [ctypes.c_int] * 6 + [_P, _P]),
    "vp_maxpool_hw": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, _P]),
    "vp_gru_seq": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P]),
    "vp_bfm_reconstruct_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_bfm_reconstruct": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_bfm_reconstruct_view": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P, _P,
                                               ctypes.c_size_t, _P]),
    "vp_sheet_tile_u8": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_landmark_distance": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_bfmfit_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "vp_bfmfit_fit": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_bfmfit_identity_step": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_double, _P, ctypes.c_size_t, _P]),
    "vp_bfmfit_clip_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "vp_bfmfit_clip": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P, ctypes.c_int, _P, ctypes.c_int, _P, _P, ctypes.c_double, ctypes.c_double, _P,
                                      ctypes.c_double, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_bfmfit_observe_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_bfmfit_observe": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_bfmfit_observe_opts_size": (ctypes.c_size_t, []),
    "vp_bfmfit_observe_ex_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_bfmfit_observe_ex": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P,
                                            ctypes.c_size_t, _P, _P, _P]),
    "vp_bfmfit_appearance_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "vp_bfmfit_appearance": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "vp_render_colors_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_render_colors": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, _P, _P]),
    "vp_rasterize_triangles_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_rasterize_triangles": (ctypes.c_int, [_P] * 5 + [ctypes.c_int] * 5 + [_P, _P]),
    "vp_render_texture_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_render_texture": (ctypes.c_int, [_P] * 7 + [ctypes.c_int] * 12 + [_P, _P]),
    "vp_raster_interpolate": (ctypes.c_int, [_P] * 5 + [ctypes.c_int] * 6 + [_P]),
    "vp_raster_vertex_visibility": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P]),
    "vp_vertex_adjacency_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "vp_vertex_adjacency_build": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_size_t, _P]),
    "vp_vertex_normals": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_bn_train_workspace_bytes":(ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int]),
    "vp_bn_train_fwd": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.c_int, _P, ctypes.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "vp_bn_train_bwd": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int, _P, _P, _P, _P, _P, _P]),
    "vp_affine_act_fwd": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_affine_act_add_fwd": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_act_bwd": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_int, _P, _P]),
    "vp_dwconv7x3_raw": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_dwconv7x3_bwd_data": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_dwconv7x3_wgrad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vp_bn_act_train_bwd": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "vp_l2_regulariser": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_float, _P, _P]),
    "vp_adam_tf_clipped": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_size_t, _P, _P, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P]),
    "vp_moving_update": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_float, _P]),
    "vp_dwconv7x3_wgrad": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_maxpool_hw_bwd": (ctypes.c_int, [_P, _P, _P] + [ctypes.c_int] * 8 + [_P]),
    "vp_stem_im2col": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "vp_gru_train_fwd": (ctypes.c_int, [_P] * 10 + [ctypes.c_int, ctypes.c_int, _P]),
    "vp_gru_train_bwd": (ctypes.c_int, [_P] * 10 + [ctypes.c_int, ctypes.c_int, _P]),
    "vp_colsum_f32": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_gru_split_recurrent": (ctypes.c_int, [_P] * 7),
    "vp_mul_f32": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P]),
    "vp_add_ears_f32": (ctypes.c_int, [_P, _P, ctypes.c_int, _P]),
    "vp_vertex_loss_partials": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "vp_bfm_vertex_loss": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "vp_sumsq_partials": (ctypes.c_int, [ctypes.c_size_t]),
    "vp_sum_f64": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_double, _P, _P, _P]),
    "vp_bfm_step_report": (ctypes.c_int, [_P, _P, ctypes.c_double, _P, _P, _P]),
    "vp_clip_scale_f32": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_float, _P]),
    "vp_sumsq": (ctypes.c_int, [_P, ctypes.c_size_t, _P, _P]),
    "vp_bn_bwd": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "vp_bn_groups_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "vp_bn_groups_fwd": (ctypes.c_int, [_P] + [ctypes.c_int] * 4 + [_P, _P, ctypes.c_float] + [_P] * 6 + [ctypes.c_int, _P, _P]),
    "vp_bn_groups_bwd": (ctypes.c_int, [_P, _P, _P] + [ctypes.c_int] * 4 + [_P] * 8 + [ctypes.c_int, ctypes.c_int, _P, _P]),
    "vp_bn_groups_bwd_tail": (ctypes.c_int, [_P, _P, _P] + [ctypes.c_int] * 4 + [_P] * 4 + [ctypes.c_int, ctypes.c_int] + [_P] * 5 + [ctypes.c_int, _P]),
    "vp_colsum_groups": (ctypes.c_int, [_P] + [ctypes.c_int] * 5 + [_P, ctypes.c_int, _P, _P]),
    "vp_act_apply": (ctypes.c_int, [_P, _P, _P] + [ctypes.c_int] * 4 + [_P, _P, _P]),
    "vp_relu_bwd": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int, _P]),
    "vp_tap_gather": (ctypes.c_int, [_P, _P, _P] + [ctypes.c_int] * 5 + [_P]),
    "vp_tap_spread": (ctypes.c_int, [_P, ctypes.c_int, _P] + [ctypes.c_int] * 5 + [_P]),
    "vp_pack_inputs": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, _P, _P, _P] + [ctypes.c_int] * 4 + [_P]),
    "vp_composite_nblocks": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "vp_composite_fwd_train": (ctypes.c_int, [_P] * 9 + [ctypes.c_int] * 3 + [_P]),
    "vp_composite_bwd": (ctypes.c_int, [_P] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, _P]),
    "vp_perceptual_nblocks": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_int]),
    "vp_perceptual": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_float, ctypes.c_int, _P]),
    "vp_loss_final": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_float, ctypes.c_float, _P, _P]),
}

# vp_X_desc_size -> the structure that restates vp_X_desc here: lib() compares the two sizes.  A new descriptor gets its line
# (tests/test_host_logic.py lists the exported queries against this table).
DESC_SIZE_QUERIES = {
    "vp_pixrefer_desc_size": PixReferDesc,
    "vp_bfmstream_desc_size": BfmStreamDesc,
    "vp_bfmstream_group_desc_size": BfmStreamGroupDesc,
    "vp_puppet_desc_size": PuppetDesc,
    "vp_jpeg_desc_size": JpegDesc,
    "vp_png_desc_size": PngDesc,
    "vp_jpegdec_desc_size": JpegDecDesc,
    "vp_pcmin_desc_size": PcmInDesc,
    "vp_frame_metrics_desc_size": FrameMetricsDesc,
    "vp_avimux_desc_size": AviMuxDesc,
    "vp_triptych_desc_size": TriptychDesc,
    "vp_keymatte_desc_size": KeyMatteDesc,
    "vp_matteclean_desc_size": MatteCleanDesc,
    "vp_mattesolve_desc_size": MatteSolveDesc,
}

_lib = None


def lib():
  """The loaded library; raises (never falls back) when it has not been built."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise RuntimeError("libvp_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "or `make -C voicepuppet_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    # PyTorch first: it carries its own HIP runtime (torch/lib/libamdhip64.so); a process that loaded the system runtime through THIS
    # library before importing torch ends up with two runtimes, and the second finds no device ("no ROCm-capable device is detected" from
    # the first HIP call of the library - seen with __graft_entry__.build() followed by smoke() in one process).  Loaded in this order
    # the library binds to the runtime torch already mapped.
    try:
      import torch  # noqa: F401
    except ImportError:
      pass
    l = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
      try:
        fn = getattr(l, name)
      except AttributeError:
        if "VP_LIB" not in os.environ:       # the shipped library exports everything include/vp_hip.h declares (tests/test_host_logic.py)
          raise
        continue                             # an A/B build of an older tree (scripts/ab.sh): entry points added since are simply absent
      fn.restype = res
      fn.argtypes = args
    # every descriptor is declared twice (include/vp_hip.h, the structures above): a library built from another header must not be handed
    # this layout (include/vp_hip.h, "ABI rule"); an older A/B build (VP_LIB) without a query is skipped (vp_pixrefer_desc: it is the
    # 48-byte round-5 layout)
    for query, struct in DESC_SIZE_QUERIES.items():
      if hasattr(l, query) and getattr(l, query).argtypes is not None:
        want = int(getattr(l, query)())
        if want != ctypes.sizeof(struct):
          raise RuntimeError("%s: %s is %d bytes in the library, %d in this binding" % (LIB_PATH, query[:-len("_size")], want, ctypes.sizeof(struct)))
    _lib = l
  return _lib


def exported_symbols():
  return sorted(_SIGNATURES)


def check(rc, what=""):
  if rc != 0:
    raise RuntimeError("%s failed (%d): %s" % (what or "libvp_hip call", rc, lib().vp_last_error().decode()))
