"""ctypes binding of include/bhw.h (the C ABI).  Fails loudly when libbhw.so is absent."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))

MODEL_HLS, MODEL_CPP, MODEL_VHDL, MODEL_DDS48, MODEL_SCALED = 0, 1, 2, 3, 4
COMBINE_HLS, COMBINE_VHDL = 0, 1
SIN_CORDIC, SIN_TAYLOR, SIN_TAYLOR_ALL = 0, 1, 2
WIN_HAMMING, WIN_HANN, WIN_BH3, WIN_BH4, WIN_BH5, WIN_BH7 = 1, 2, 3, 4, 5, 7
ALGO_AUTO, ALGO_DIRECT, ALGO_TABLE, ALGO_FUSED = 0, 1, 2, 3
TABLE_BEST, TABLE_PLAIN, TABLE_DELTA16, TABLE_RESIDUAL, TABLE_NIBBLE, TABLE_NIBBLE_ESC = 0, 1, 2, 3, 4, 5
ABI_VERSION = 4
OLA_NORMALIZE = 1
PAD_CONSTANT, PAD_REFLECT = 0, 1        # bhw_stft.pad_mode
SUMS_F32 = 1                            # bhw_window_sums_* flags
WELCH_DETREND_CONSTANT = 1              # bhw_welch_frames_f32_* flags
PSD_ONESIDED = 1                        # bhw_psd.flags
WELCH_BLOCK = 256                       # BHW_WELCH_BLOCK: frames of one block of the periodogram sum
CSD_ONESIDED, CSD_BROADCAST_X = 1, 2    # bhw_csd.flags
CSD_PXY, CSD_PXX, CSD_PYY, CSD_COHERENCE, CSD_H1 = 0x10, 0x20, 0x40, 0x80, 0x100
# output name -> (flag, complex); the order of the pointers of bhw_welch_csd_f32
CSD_OUTPUTS = {"pxy": (CSD_PXY, True), "pxx": (CSD_PXX, False), "pyy": (CSD_PYY, False), "coherence": (CSD_COHERENCE, False),
               "h1": (CSD_H1, True)}

# every symbol include/bhw.h declares (tests check the library exports all of them)
ABI_SYMBOLS = (
    "bhw_abi_version", "bhw_strerror", "bhw_last_error", "bhw_params_init", "bhw_params_validate",
    "bhw_coeffs_from_float", "bhw_constant_tables", "bhw_generate_device", "bhw_generate_device_ex",
    "bhw_workspace_bytes", "bhw_generate_batched_device", "bhw_sincos_device", "bhw_generate_to_host",
    "bhw_sincos_to_host", "bhw_release_device", "bhw_apply_device", "bhw_atan2_device", "bhw_atan2_to_host",
    "bhw_prepare_device", "bhw_part_segments", "bhw_generate_part_device", "bhw_describe_plan",
    "bhw_coeffs_preset", "bhw_gather_parts_device", "bhw_workspace_bytes_ex",
    "bhw_table_create", "bhw_table_destroy", "bhw_table_bytes", "bhw_table_describe", "bhw_generate_from_table",
    "bhw_apply_from_table", "bhw_generate_part_from_table",
    "bhw_apply_frames_device", "bhw_apply_frames_from_table", "bhw_apply_frames_describe",
    "bhw_overlap_add_device", "bhw_overlap_add_from_table", "bhw_overlap_add_describe",
    "bhw_generate_len_device", "bhw_generate_len_from_table", "bhw_apply_frames_len_device", "bhw_apply_frames_len_from_table",
    "bhw_overlap_add_len_device", "bhw_overlap_add_len_from_table", "bhw_describe_len",
    "bhw_apply_frames_f32_device", "bhw_apply_frames_f32_from_table", "bhw_overlap_add_f32_device", "bhw_overlap_add_f32_from_table",
    "bhw_describe_f32",
    "bhw_stft_frames_f32_device", "bhw_stft_frames_f32_from_table", "bhw_istft_ola_f32_device", "bhw_istft_ola_f32_from_table",
    "bhw_describe_stft",
    "bhw_window_sums_device", "bhw_window_sums_from_table", "bhw_welch_workspace_bytes", "bhw_welch_frames_f32_device",
    "bhw_welch_frames_f32_from_table", "bhw_welch_psd_workspace_bytes", "bhw_welch_psd_f32", "bhw_describe_welch",
    "bhw_welch_csd_workspace_bytes", "bhw_welch_csd_f32", "bhw_describe_csd",
    "bhw_stft_fft_f32_device", "bhw_stft_fft_f32_from_table", "bhw_describe_stft_fft",
    "bhw_istft_fft_f32_device", "bhw_istft_fft_f32_from_table", "bhw_describe_istft_fft",
    "bhw_spectrogram_f32_device", "bhw_spectrogram_f32_from_table", "bhw_describe_spectrogram",
    "bhw_stft_mfft_f32_device", "bhw_stft_mfft_f32_from_table", "bhw_describe_stft_mfft",
    "bhw_logspec_f32_device", "bhw_logspec_f32_from_table", "bhw_describe_logspec",
    "bhw_logspec_mfft_f32_device", "bhw_logspec_mfft_f32_from_table", "bhw_describe_logspec_mfft",
    "bhw_istft_mfft_f32_device", "bhw_istft_mfft_f32_from_table", "bhw_describe_istft_mfft",
    "bhw_stft_cfft_f32_device", "bhw_stft_cfft_f32_from_table", "bhw_describe_stft_cfft",
    "bhw_istft_cfft_f32_device", "bhw_istft_cfft_f32_from_table", "bhw_describe_istft_cfft",
    "bhw_stft_cmfft_f32_device", "bhw_stft_cmfft_f32_from_table", "bhw_describe_stft_cmfft",
    "bhw_istft_cmfft_f32_device", "bhw_istft_cmfft_f32_from_table", "bhw_describe_istft_cmfft",
    "bhw_welch_fft_workspace_bytes", "bhw_welch_fft_f32_device", "bhw_welch_fft_f32_from_table", "bhw_describe_welch_fft",
    "bhw_csd_fft_workspace_bytes", "bhw_csd_fft_f32_device", "bhw_csd_fft_f32_from_table", "bhw_describe_csd_fft",
    "bhw_welch_cfft_workspace_bytes", "bhw_welch_cfft_f32_device", "bhw_welch_cfft_f32_from_table", "bhw_describe_welch_cfft",
    "bhw_welch_mfft_workspace_bytes", "bhw_welch_mfft_f32_device", "bhw_welch_mfft_f32_from_table", "bhw_describe_welch_mfft",
    "bhw_welch_cmfft_workspace_bytes", "bhw_welch_cmfft_f32_device", "bhw_welch_cmfft_f32_from_table", "bhw_describe_welch_cmfft",
    "bhw_hold_cfft_workspace_bytes", "bhw_hold_cfft_f32_device", "bhw_hold_cfft_f32_from_table", "bhw_describe_hold_cfft",
    "bhw_hold_cmfft_workspace_bytes", "bhw_hold_cmfft_f32_device", "bhw_hold_cmfft_f32_from_table", "bhw_describe_hold_cmfft",
    "bhw_hold_fft_workspace_bytes", "bhw_hold_fft_f32_device", "bhw_hold_fft_f32_from_table", "bhw_describe_hold_fft",
    "bhw_hold_mfft_workspace_bytes", "bhw_hold_mfft_f32_device", "bhw_hold_mfft_f32_from_table", "bhw_describe_hold_mfft",
    "bhw_mask_fft_f32_device", "bhw_mask_fft_f32_from_table", "bhw_describe_mask_fft",
    "bhw_mask_mfft_f32_device", "bhw_mask_mfft_f32_from_table", "bhw_describe_mask_mfft",
    "bhw_cmask_fft_f32_device", "bhw_cmask_fft_f32_from_table", "bhw_describe_cmask_fft",
    "bhw_cmask_mfft_f32_device", "bhw_cmask_mfft_f32_from_table", "bhw_describe_cmask_mfft",
    "bhw_mask_cfft_f32_device", "bhw_mask_cfft_f32_from_table", "bhw_describe_mask_cfft",
    "bhw_cmask_cfft_f32_device", "bhw_cmask_cfft_f32_from_table", "bhw_describe_cmask_cfft",
    "bhw_mask_cmfft_f32_device", "bhw_mask_cmfft_f32_from_table", "bhw_describe_mask_cmfft",
    "bhw_cmask_cmfft_f32_device", "bhw_cmask_cmfft_f32_from_table", "bhw_describe_cmask_cmfft",
    "bhw_beam_fft_f32_device", "bhw_beam_fft_f32_from_table", "bhw_describe_beam_fft",
    "bhw_beam_mfft_f32_device", "bhw_beam_mfft_f32_from_table", "bhw_describe_beam_mfft",
)


class BhwError(RuntimeError):
    def __init__(self, code, detail):
        super().__init__(f"bhw error {code}: {detail}")
        self.code = code
        self.detail = detail


class BhwParams(ctypes.Structure):
    """struct bhw_params of include/bhw.h (the win_selector parameter surface)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("model", ctypes.c_uint32), ("combine", ctypes.c_uint32),
        ("sin_type", ctypes.c_uint32), ("win_type", ctypes.c_uint32), ("n_terms", ctypes.c_uint32),
        ("phi_width", ctypes.c_uint32), ("dat_width", ctypes.c_uint32), ("precision", ctypes.c_uint32),
        ("lut_size", ctypes.c_uint32), ("aa", ctypes.c_int32 * 7),
    ]


class BhwAtan2Params(ctypes.Structure):
    """struct bhw_atan2_params of include/bhw.h (generics of entity cordic_atan2, src/cordic_atan2.vhd:64-69)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("precision", ctypes.c_uint32),
                ("input_width", ctypes.c_uint32), ("angle_width", ctypes.c_uint32)]


class BhwSegment(ctypes.Structure):
    _fields_ = [("n0", ctypes.c_uint64), ("count", ctypes.c_uint64)]


class BhwExec(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("algo", ctypes.c_uint32),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_uint64),
                ("event_after_build", ctypes.c_void_p), ("table_format", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BhwFrames(ctypes.Structure):
    """struct bhw_frames of include/bhw.h (the overlapped-frame apply)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("frames", ctypes.c_uint64),
                ("hop", ctypes.c_uint64), ("y_stride", ctypes.c_uint64), ("shift", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def make_frames(frames, hop, *, channels=1, shift=0, y_stride=0):
    f = BhwFrames()
    f.struct_size = ctypes.sizeof(BhwFrames)
    f.channels, f.frames, f.hop, f.y_stride, f.shift = int(channels), int(frames), int(hop), int(y_stride), int(shift)
    return f


class BhwOla(ctypes.Structure):
    """struct bhw_ola of include/bhw.h (the weighted overlap-add)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("frames", ctypes.c_uint64),
                ("hop", ctypes.c_uint64), ("y_stride", ctypes.c_uint64), ("t0", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("shift", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def make_ola(frames, hop, count, *, t0=0, channels=1, shift=0, y_stride=0):
    o = BhwOla()
    o.struct_size = ctypes.sizeof(BhwOla)
    o.channels, o.frames, o.hop, o.y_stride = int(channels), int(frames), int(hop), int(y_stride)
    o.t0, o.count, o.shift = int(t0), int(count), int(shift)
    return o


class BhwStft(ctypes.Structure):
    """struct bhw_stft of include/bhw.h (the batched, centred STFT framing and overlap-add)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("batch", ctypes.c_uint64),
                ("samples", ctypes.c_uint64), ("x_stride", ctypes.c_uint64), ("frames", ctypes.c_uint64), ("hop", ctypes.c_uint64),
                ("n_fft", ctypes.c_uint64), ("col0", ctypes.c_uint64), ("pad", ctypes.c_uint64), ("y_stride", ctypes.c_uint64),
                ("y_batch_stride", ctypes.c_uint64), ("pad_mode", ctypes.c_uint32), ("shift", ctypes.c_uint32)]


def make_stft(batch, samples, frames, hop, n_fft, *, col0=0, pad=0, pad_mode=0, channels=1, shift=0, x_stride=0, y_stride=0,
              y_batch_stride=0):
    s = BhwStft()
    s.struct_size = ctypes.sizeof(BhwStft)
    s.channels, s.batch, s.samples, s.frames, s.hop, s.n_fft = int(channels), int(batch), int(samples), int(frames), int(hop), int(n_fft)
    s.col0, s.pad, s.pad_mode, s.shift = int(col0), int(pad), int(pad_mode), int(shift)
    s.x_stride, s.y_stride, s.y_batch_stride = int(x_stride), int(y_stride), int(y_batch_stride)
    return s


class BhwFbank(ctypes.Structure):
    """struct bhw_fbank of include/bhw.h (the sparse filter bank of the fused spectrogram)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("filters", ctypes.c_uint32), ("bins", ctypes.c_uint32), ("weights", ctypes.c_uint32),
                ("d_first", ctypes.c_void_p), ("d_offset", ctypes.c_void_p), ("d_weight", ctypes.c_void_p), ("reserved", ctypes.c_uint64)]


def make_fbank(filters, bins, weights, d_first, d_offset, d_weight):
    """A bhw_fbank over three device arrays given as addresses (ints or None): d_first (filters uint32), d_offset (filters + 1
    uint32) and d_weight (weights float32)."""
    fb = BhwFbank()
    fb.struct_size = ctypes.sizeof(BhwFbank)
    fb.filters, fb.bins, fb.weights = int(filters), int(bins), int(weights)
    fb.d_first, fb.d_offset, fb.d_weight = d_first, d_offset, d_weight
    return fb


LOG_CLAMP, LOG_ADD = 0, 1                # BHW_LOG_CLAMP, BHW_LOG_ADD
LOG_MAX_COEFFS, LOG_MAX_DCT = 4096, 1 << 24


class BhwLogspec(ctypes.Structure):
    """struct bhw_logspec of include/bhw.h (the log and DCT stages of the fused log spectrogram / MFCC)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("floor", ctypes.c_double), ("mult", ctypes.c_double),
                ("coeffs", ctypes.c_uint32), ("dct_rows", ctypes.c_uint32), ("d_dct", ctypes.c_void_p), ("reserved", ctypes.c_uint64)]


def make_logspec(floor, mult, *, add=False, coeffs=0, dct_rows=0, d_dct=None):
    """A bhw_logspec: clamp at `floor` (or add it, add=True), mult * ln; coeffs > 0 with the (dct_rows, coeffs) float32 matrix at the
    device address d_dct (an int) for the DCT stage."""
    ls = BhwLogspec()
    ls.struct_size = ctypes.sizeof(BhwLogspec)
    ls.mode, ls.floor, ls.mult = (LOG_ADD if add else LOG_CLAMP), float(floor), float(mult)
    ls.coeffs, ls.dct_rows, ls.d_dct = int(coeffs), int(dct_rows), d_dct
    return ls


class BhwPsd(ctypes.Structure):
    """struct bhw_psd of include/bhw.h (the averaged periodogram)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("batch", ctypes.c_uint64), ("frames", ctypes.c_uint64),
                ("bins", ctypes.c_uint64), ("n_fft", ctypes.c_uint64), ("y_stride", ctypes.c_uint64), ("y_batch_stride", ctypes.c_uint64),
                ("p_stride", ctypes.c_uint64), ("scale", ctypes.c_double)]


def make_psd(batch, frames, bins, n_fft, scale, *, onesided=False, y_stride=0, y_batch_stride=0, p_stride=0):
    d = BhwPsd()
    d.struct_size = ctypes.sizeof(BhwPsd)
    d.flags = PSD_ONESIDED if onesided else 0
    d.batch, d.frames, d.bins, d.n_fft = int(batch), int(frames), int(bins), int(n_fft)
    d.y_stride, d.y_batch_stride, d.p_stride, d.scale = int(y_stride), int(y_batch_stride), int(p_stride), float(scale)
    return d


class BhwCsd(ctypes.Structure):
    """struct bhw_csd of include/bhw.h (the Welch cross spectra)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("batch", ctypes.c_uint64), ("frames", ctypes.c_uint64),
                ("bins", ctypes.c_uint64), ("n_fft", ctypes.c_uint64), ("x_stride", ctypes.c_uint64), ("x_batch_stride", ctypes.c_uint64),
                ("y_stride", ctypes.c_uint64), ("y_batch_stride", ctypes.c_uint64), ("o_stride", ctypes.c_uint64),
                ("scale", ctypes.c_double), ("reserved", ctypes.c_uint64)]


def csd_mask(outputs):
    """The output mask of bhw_csd.flags from output names (CSD_OUTPUTS)."""
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or any(o not in CSD_OUTPUTS for o in outputs):
        raise ValueError(f"outputs must be a non-empty selection, without repeats, of {tuple(CSD_OUTPUTS)}, got {outputs!r}")
    mask = 0
    for o in outputs:
        mask |= CSD_OUTPUTS[o][0]
    return mask


def make_csd(batch, frames, bins, n_fft, scale, *, outputs=("pxy",), onesided=False, broadcast_x=False, x_stride=0, x_batch_stride=0,
             y_stride=0, y_batch_stride=0, o_stride=0):
    d = BhwCsd()
    d.struct_size = ctypes.sizeof(BhwCsd)
    d.flags = csd_mask(outputs) | (CSD_ONESIDED if onesided else 0) | (CSD_BROADCAST_X if broadcast_x else 0)
    d.batch, d.frames, d.bins, d.n_fft = int(batch), int(frames), int(bins), int(n_fft)
    d.x_stride, d.x_batch_stride, d.y_stride, d.y_batch_stride = int(x_stride), int(x_batch_stride), int(y_stride), int(y_batch_stride)
    d.o_stride, d.scale = int(o_stride), float(scale)
    return d


_lib = None


def lib_path():
    return os.path.join(HERE, "libbhw.so")


def lib():
    """The loaded C-ABI library.  Raises (no fallback) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m blackman_harris_win_amd._build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch owns the device memory and streams handed to the ABI, so its HIP runtime must be the one this
    # process uses: import it before libbhw.so pulls in libamdhip64 (two runtimes in one process do not
    # share devices or pointers).  A C/C++ host that links libbhw.so directly needs no torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    P = ctypes.POINTER(BhwParams)
    u32, u64, i32p, vp, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int
    L.bhw_abi_version.restype = u32
    L.bhw_strerror.restype = ctypes.c_char_p
    L.bhw_strerror.argtypes = [ci]
    L.bhw_last_error.restype = ctypes.c_char_p
    L.bhw_params_init.argtypes = [P, u32, u32, u32]
    L.bhw_params_validate.argtypes = [P]
    L.bhw_coeffs_from_float.argtypes = [u32, u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.bhw_constant_tables.argtypes = [u32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.bhw_coeffs_preset.argtypes = [u32, u32, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.bhw_gather_parts_device.argtypes = [P, u32, ctypes.POINTER(ci), ctypes.POINTER(vp), ci, vp, i32p]
    L.bhw_generate_device.argtypes = [P, ci, vp, u64, u64, i32p]
    L.bhw_generate_device_ex.argtypes = [P, ci, vp, u64, u64, i32p, ctypes.POINTER(BhwExec)]
    L.bhw_workspace_bytes.restype = u64
    L.bhw_workspace_bytes.argtypes = [P, u64, u64, u32]
    L.bhw_workspace_bytes_ex.restype = u64
    L.bhw_workspace_bytes_ex.argtypes = [P, u64, u64, ctypes.POINTER(BhwExec)]
    L.bhw_generate_batched_device.argtypes = [P, ci, vp, u32, i32p]
    L.bhw_sincos_device.argtypes = [P, ci, vp, u64, u64, i32p, i32p]
    L.bhw_generate_to_host.argtypes = [P, ci, u64, u64, i32p]
    L.bhw_sincos_to_host.argtypes = [P, ci, u64, u64, i32p, i32p]
    L.bhw_release_device.argtypes = [ci]
    L.bhw_prepare_device.argtypes = [P, ci, vp]
    L.bhw_describe_plan.argtypes = [P, u64, u64, ctypes.POINTER(BhwExec), ctypes.c_char_p, u64]
    L.bhw_part_segments.argtypes = [P, u32, u32, ctypes.POINTER(BhwSegment), u32, ctypes.POINTER(u32)]
    L.bhw_generate_part_device.argtypes = [P, ci, vp, u32, u32, i32p, ctypes.POINTER(BhwExec)]
    L.bhw_apply_device.argtypes = [P, ci, vp, u64, u64, i32p, i32p, u32]
    T = ctypes.c_void_p                                     # bhw_table (opaque handle)
    L.bhw_table_create.argtypes = [P, ci, vp, u32, ctypes.POINTER(T)]
    L.bhw_table_destroy.argtypes = [T]
    L.bhw_table_bytes.restype = u64
    L.bhw_table_bytes.argtypes = [T]
    L.bhw_table_describe.argtypes = [T, P, u64, u64, ctypes.c_char_p, u64]
    L.bhw_generate_from_table.argtypes = [T, P, vp, u64, u64, i32p]
    L.bhw_apply_from_table.argtypes = [T, P, vp, u64, u64, i32p, i32p, u32]
    L.bhw_generate_part_from_table.argtypes = [T, P, vp, u32, u32, i32p]
    L.bhw_dbg_table_key_matches.argtypes = [P, P]
    L.bhw_dbg_describe_from_table.argtypes = [P, u32, P, u64, u64, ctypes.c_char_p, u64]
    L.bhw_dbg_generate_from_table_generic.argtypes = [T, P, vp, u64, u64, i32p]
    F = ctypes.POINTER(BhwFrames)
    L.bhw_apply_frames_device.argtypes = [P, ci, vp, F, i32p, i32p]
    L.bhw_apply_frames_from_table.argtypes = [T, P, vp, F, i32p, i32p]
    L.bhw_apply_frames_describe.argtypes = [T, P, F, ctypes.c_char_p, u64]
    L.bhw_dbg_apply_frames_route.argtypes = [P, ci, vp, F, i32p, i32p, ci]
    L.bhw_dbg_describe_frames_from_table.argtypes = [P, u32, P, F, ctypes.c_char_p, u64]
    O = ctypes.POINTER(BhwOla)
    L.bhw_overlap_add_device.argtypes = [P, ci, vp, O, i32p, i32p]
    L.bhw_overlap_add_from_table.argtypes = [T, P, vp, O, i32p, i32p]
    L.bhw_overlap_add_describe.argtypes = [T, P, O, ctypes.c_char_p, u64]
    L.bhw_dbg_overlap_add_shape.argtypes = [T, P, ci, vp, O, i32p, i32p, u32, u32]
    L.bhw_dbg_describe_ola_from_table.argtypes = [P, u32, P, O, ctypes.c_char_p, u64]
    L.bhw_generate_len_device.argtypes = [P, u64, ci, vp, u64, u64, i32p]
    L.bhw_generate_len_from_table.argtypes = [T, P, u64, vp, u64, u64, i32p]
    L.bhw_apply_frames_len_device.argtypes = [P, u64, ci, vp, F, i32p, i32p]
    L.bhw_apply_frames_len_from_table.argtypes = [T, P, u64, vp, F, i32p, i32p]
    L.bhw_overlap_add_len_device.argtypes = [P, u64, ci, vp, O, i32p, i32p]
    L.bhw_overlap_add_len_from_table.argtypes = [T, P, u64, vp, O, i32p, i32p]
    L.bhw_describe_len.argtypes = [T, P, u64, u64, u64, F, O, ctypes.c_char_p, u64]
    L.bhw_dbg_len_force_kernels.argtypes = [ci]
    f32p = ctypes.c_void_p
    L.bhw_apply_frames_f32_device.argtypes = [P, u64, ci, vp, F, f32p, f32p]
    L.bhw_apply_frames_f32_from_table.argtypes = [T, P, u64, vp, F, f32p, f32p]
    L.bhw_overlap_add_f32_device.argtypes = [P, u64, ci, vp, O, u32, f32p, f32p]
    L.bhw_overlap_add_f32_from_table.argtypes = [T, P, u64, vp, O, u32, f32p, f32p]
    L.bhw_describe_f32.argtypes = [T, P, u64, F, O, u32, ctypes.c_char_p, u64]
    S = ctypes.POINTER(BhwStft)
    L.bhw_stft_frames_f32_device.argtypes = [P, u64, ci, vp, S, f32p, f32p]
    L.bhw_stft_frames_f32_from_table.argtypes = [T, P, u64, vp, S, f32p, f32p]
    L.bhw_istft_ola_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_istft_ola_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_stft.argtypes = [T, P, u64, S, ci, u32, ctypes.c_char_p, u64]
    D = ctypes.POINTER(BhwPsd)
    L.bhw_window_sums_device.argtypes = [P, u64, ci, vp, u32, vp]
    L.bhw_window_sums_from_table.argtypes = [T, P, u64, vp, u32, vp]
    L.bhw_welch_workspace_bytes.restype = u64
    L.bhw_welch_workspace_bytes.argtypes = [S, u32]
    L.bhw_welch_frames_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p, vp, u64]
    L.bhw_welch_frames_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p, vp, u64]
    L.bhw_welch_psd_workspace_bytes.restype = u64
    L.bhw_welch_psd_workspace_bytes.argtypes = [D]
    L.bhw_welch_psd_f32.argtypes = [ci, vp, D, f32p, f32p, vp, u64]
    L.bhw_describe_welch.argtypes = [T, P, u64, S, u32, D, ctypes.c_char_p, u64]
    X = ctypes.POINTER(BhwCsd)
    L.bhw_welch_csd_workspace_bytes.restype = u64
    L.bhw_welch_csd_workspace_bytes.argtypes = [X]
    L.bhw_welch_csd_f32.argtypes = [ci, vp, X, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp, u64]
    L.bhw_describe_csd.argtypes = [X, ctypes.c_char_p, u64]
    L.bhw_stft_fft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_stft_fft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_stft_fft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_istft_fft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_istft_fft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_istft_fft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_mask_fft_f32_device.argtypes = [P, u64, ci, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
    L.bhw_mask_fft_f32_from_table.argtypes = [T, P, u64, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
    L.bhw_describe_mask_fft.argtypes = [T, P, u64, S, S, u32, u64, u64, ctypes.c_char_p, u64]
    L.bhw_mask_mfft_f32_device.argtypes = [P, u64, ci, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
    L.bhw_mask_mfft_f32_from_table.argtypes = [T, P, u64, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
    L.bhw_describe_mask_mfft.argtypes = [T, P, u64, S, S, u32, u64, u64, ctypes.c_char_p, u64]
    for fam in ("fft", "mfft"):                          # d_g: interleaved float32 pairs, the strides in pairs
        getattr(L, f"bhw_cmask_{fam}_f32_device").argtypes = [P, u64, ci, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
        getattr(L, f"bhw_cmask_{fam}_f32_from_table").argtypes = [T, P, u64, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
        getattr(L, f"bhw_describe_cmask_{fam}").argtypes = [T, P, u64, S, S, u32, u64, u64, ctypes.c_char_p, u64]
    for fam in ("fft", "mfft"):                          # filter-and-sum: n_ch and x_ch_stride behind d_x, g_ch_stride between the gain strides
        getattr(L, f"bhw_beam_{fam}_f32_device").argtypes = [P, u64, ci, vp, S, S, u32, f32p, u32, u64, f32p, u64, u64, u64, f32p]
        getattr(L, f"bhw_beam_{fam}_f32_from_table").argtypes = [T, P, u64, vp, S, S, u32, f32p, u32, u64, f32p, u64, u64, u64, f32p]
        getattr(L, f"bhw_describe_beam_{fam}").argtypes = [T, P, u64, S, S, u32, u32, u64, u64, u64, u64, ctypes.c_char_p, u64]
    for name in ("mask_cfft", "cmask_cfft", "mask_cmfft", "cmask_cmfft"):          # the same twelve for I/Q input
        getattr(L, f"bhw_{name}_f32_device").argtypes = [P, u64, ci, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
        getattr(L, f"bhw_{name}_f32_from_table").argtypes = [T, P, u64, vp, S, S, u32, f32p, f32p, u64, u64, f32p]
        getattr(L, f"bhw_describe_{name}").argtypes = [T, P, u64, S, S, u32, u64, u64, ctypes.c_char_p, u64]
    FB = ctypes.POINTER(BhwFbank)
    L.bhw_spectrogram_f32_device.argtypes = [P, u64, ci, vp, S, u32, FB, f32p, f32p]
    L.bhw_spectrogram_f32_from_table.argtypes = [T, P, u64, vp, S, u32, FB, f32p, f32p]
    L.bhw_describe_spectrogram.argtypes = [T, P, u64, S, u32, FB, ctypes.c_char_p, u64]
    L.bhw_stft_mfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, FB, f32p, f32p]
    L.bhw_stft_mfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, FB, f32p, f32p]
    L.bhw_describe_stft_mfft.argtypes = [T, P, u64, S, u32, FB, ctypes.c_char_p, u64]
    LS = ctypes.POINTER(BhwLogspec)
    for stem in ("bhw_logspec", "bhw_logspec_mfft"):
        getattr(L, stem + "_f32_device").argtypes = [P, u64, ci, vp, S, u32, FB, LS, f32p, f32p]
        getattr(L, stem + "_f32_from_table").argtypes = [T, P, u64, vp, S, u32, FB, LS, f32p, f32p]
        getattr(L, "bhw_describe_" + stem[4:]).argtypes = [T, P, u64, S, u32, FB, LS, ctypes.c_char_p, u64]
    L.bhw_istft_mfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_istft_mfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_istft_mfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_stft_cfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, vp, vp]
    L.bhw_stft_cfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, vp, vp]
    L.bhw_describe_stft_cfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_stft_cmfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, vp, vp]
    L.bhw_stft_cmfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, vp, vp]
    L.bhw_describe_stft_cmfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_istft_cfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_istft_cfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_istft_cfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_istft_cmfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f32p, f32p]
    L.bhw_istft_cmfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f32p, f32p]
    L.bhw_describe_istft_cmfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    f64 = ctypes.c_double
    L.bhw_welch_fft_workspace_bytes.restype = u64
    L.bhw_welch_fft_workspace_bytes.argtypes = [S]
    L.bhw_welch_fft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f64, u32, f32p, f32p, u64, vp, u64]
    L.bhw_welch_fft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f64, u32, f32p, f32p, u64, vp, u64]
    L.bhw_describe_welch_fft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_csd_fft_workspace_bytes.restype = u64
    L.bhw_csd_fft_workspace_bytes.argtypes = [S]
    L.bhw_csd_fft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f64, u32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, u64, vp, u64]
    L.bhw_csd_fft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f64, u32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, u64, vp, u64]
    L.bhw_describe_csd_fft.argtypes = [T, P, u64, S, u32, u32, ctypes.c_char_p, u64]
    L.bhw_welch_cfft_workspace_bytes.restype = u64
    L.bhw_welch_cfft_workspace_bytes.argtypes = [S]
    L.bhw_welch_cfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f64, f32p, f32p, u64, vp, u64]
    L.bhw_welch_cfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f64, f32p, f32p, u64, vp, u64]
    L.bhw_describe_welch_cfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_welch_mfft_workspace_bytes.restype = u64
    L.bhw_welch_mfft_workspace_bytes.argtypes = [S]
    L.bhw_welch_mfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f64, u32, f32p, f32p, u64, vp, u64]
    L.bhw_welch_mfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f64, u32, f32p, f32p, u64, vp, u64]
    L.bhw_describe_welch_mfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    L.bhw_welch_cmfft_workspace_bytes.restype = u64
    L.bhw_welch_cmfft_workspace_bytes.argtypes = [S]
    L.bhw_welch_cmfft_f32_device.argtypes = [P, u64, ci, vp, S, u32, f64, f32p, f32p, u64, vp, u64]
    L.bhw_welch_cmfft_f32_from_table.argtypes = [T, P, u64, vp, S, u32, f64, f32p, f32p, u64, vp, u64]
    L.bhw_describe_welch_cmfft.argtypes = [T, P, u64, S, u32, ctypes.c_char_p, u64]
    for fam in ("cfft", "cmfft"):
        getattr(L, f"bhw_hold_{fam}_workspace_bytes").restype = u64
        getattr(L, f"bhw_hold_{fam}_workspace_bytes").argtypes = [S]
        getattr(L, f"bhw_hold_{fam}_f32_device").argtypes = [P, u64, ci, vp, S, u32, f64, f32p, f32p, f32p, u64, vp, u64]
        getattr(L, f"bhw_hold_{fam}_f32_from_table").argtypes = [T, P, u64, vp, S, u32, f64, f32p, f32p, f32p, u64, vp, u64]
        getattr(L, f"bhw_describe_hold_{fam}").argtypes = [T, P, u64, S, u32, u32, ctypes.c_char_p, u64]
    for fam in ("fft", "mfft"):                                  # real input: the Welch siblings' lists with two outputs for d_P
        getattr(L, f"bhw_hold_{fam}_workspace_bytes").restype = u64
        getattr(L, f"bhw_hold_{fam}_workspace_bytes").argtypes = [S]
        getattr(L, f"bhw_hold_{fam}_f32_device").argtypes = [P, u64, ci, vp, S, u32, f64, u32, f32p, f32p, f32p, u64, vp, u64]
        getattr(L, f"bhw_hold_{fam}_f32_from_table").argtypes = [T, P, u64, vp, S, u32, f64, u32, f32p, f32p, f32p, u64, vp, u64]
        getattr(L, f"bhw_describe_hold_{fam}").argtypes = [T, P, u64, S, u32, u32, ctypes.c_char_p, u64]
    PA = ctypes.POINTER(BhwAtan2Params)
    L.bhw_atan2_device.argtypes = [PA, ci, vp, u64, i32p, i32p, i32p]
    L.bhw_atan2_to_host.argtypes = [PA, ci, u64, i32p, i32p, i32p]
    if L.bhw_abi_version() != ABI_VERSION:
        raise ImportError(f"{path} has ABI version {L.bhw_abi_version()}, this binding needs {ABI_VERSION}: rebuild it "
                          "(`python -m blackman_harris_win_amd._build --force`)")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise BhwError(rc, lib().bhw_last_error().decode(errors="replace"))


def describe_plan(params, n0, count, algo=ALGO_AUTO, table_format=TABLE_BEST):
    """One line: strategy, table format and kernel names a call would launch now (bhw_describe_plan)."""
    ex = BhwExec()
    ex.struct_size = ctypes.sizeof(BhwExec)
    ex.algo = algo
    ex.table_format = table_format
    buf = ctypes.create_string_buffer(256)
    check(lib().bhw_describe_plan(ctypes.byref(params), int(n0), int(count), ctypes.byref(ex), buf, 256))
    return buf.value.decode()


def describe_table(table, params, n0, count):
    """One line: the resident table's format, layout and bytes, and the kernels a from-table call of (params, n0, count) launches
    (bhw_table_describe; `table` is the handle, e.g. ResidentTable.handle)."""
    buf = ctypes.create_string_buffer(384)
    check(lib().bhw_table_describe(table, ctypes.byref(params), int(n0), int(count), buf, 384))
    return buf.value.decode()


def describe_frames(params, frames, hop, *, channels=1, y_stride=0, table=None):
    """One line: the route, the frame-group size and the kernels an overlapped-frame apply would launch (bhw_apply_frames_describe;
    `table` is a resident table handle or None for the library call).  Host arithmetic only."""
    buf = ctypes.create_string_buffer(384)
    f = make_frames(frames, hop, channels=channels, y_stride=y_stride)
    check(lib().bhw_apply_frames_describe(table, ctypes.byref(params), ctypes.byref(f), buf, 384))
    return buf.value.decode()


def describe_ola(params, frames, hop, count=None, *, t0=0, channels=1, y_stride=0, table=None):
    """One line: the route, Q, the lane layout, the grid and the kernel an overlap-add would launch (bhw_overlap_add_describe;
    `table` is a resident table handle or None for the library call; count=None: the whole extent).  Host arithmetic only."""
    if count is None:
        count = max(0, (int(frames) - 1) * int(hop) + (1 << params.phi_width) - int(t0)) if frames else 0
    buf = ctypes.create_string_buffer(384)
    o = make_ola(frames, hop, count, t0=t0, channels=channels, y_stride=y_stride)
    check(lib().bhw_overlap_add_describe(table, ctypes.byref(params), ctypes.byref(o), buf, 384))
    return buf.value.decode()


def describe_len(params, length, *, n0=0, count=None, frames=None, ola=None, table=None):
    """One line: the route (power-of-two or any-length), kernel and grid a call for a window of `length` takes (bhw_describe_len).
    frames: a BhwFrames (make_frames) for the frames call, ola: a BhwOla (make_ola) for the overlap-add, neither: generate
    [n0, n0 + count) (count=None: one period).  `table` is a resident table handle or None for the library call.  Host arithmetic."""
    if frames is not None and ola is not None:
        raise ValueError("pass frames or ola, not both")
    count = int(length) if count is None else int(count)
    buf = ctypes.create_string_buffer(512)
    check(lib().bhw_describe_len(table, ctypes.byref(params), int(length), int(n0), count,
                                 ctypes.byref(frames) if frames is not None else None, ctypes.byref(ola) if ola is not None else None,
                                 buf, 512))
    return buf.value.decode()


def describe_f32(params, length=None, *, frames=None, ola=None, normalize=False, table=None):
    """One line: the route, the plan, the kernel and (overlap-add) whether it normalises, for a float32 call over the window of
    `length` (None: 2^phi_width) (bhw_describe_f32).  Exactly one of frames (a BhwFrames, make_frames) and ola (a BhwOla,
    make_ola).  `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    if (frames is None) == (ola is None):
        raise ValueError("pass frames or ola (one of them)")
    length = (1 << params.phi_width) if length is None else int(length)
    buf = ctypes.create_string_buffer(512)
    check(lib().bhw_describe_f32(table, ctypes.byref(params), length,
                                 ctypes.byref(frames) if frames is not None else None, ctypes.byref(ola) if ola is not None else None,
                                 OLA_NORMALIZE if normalize else 0, buf, 512))
    return buf.value.decode()


def describe_stft(params, length, stft, *, inverse=False, normalize=False, table=None):
    """One line: the route, the plan and the kernel of a batched STFT frames call (inverse False) or overlap-add (inverse True) over
    the window of `length`, for the descriptor `stft` (a BhwStft, make_stft) (bhw_describe_stft).  `table` is a resident table handle
    or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(640)
    check(lib().bhw_describe_stft(table, ctypes.byref(params), int(length), ctypes.byref(stft), 1 if inverse else 0,
                                  OLA_NORMALIZE if normalize else 0, buf, 640))
    return buf.value.decode()


def describe_welch(params=None, length=0, *, stft=None, detrend=False, psd=None, sums_f32=False, table=None):
    """One line naming the route, the plan and the kernels of a Welch call (bhw_describe_welch): the segments call of the descriptor
    `stft` (a BhwStft with pad 0, col0 0; detrend: BHW_WELCH_DETREND_CONSTANT), the periodogram of `psd` (a BhwPsd, make_psd), or,
    with neither, the window sums of the window of `length` (sums_f32: BHW_SUMS_F32).  `table` is a resident table handle or None."""
    buf = ctypes.create_string_buffer(1024)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) if stft is not None else (SUMS_F32 if sums_f32 else 0)
    check(lib().bhw_describe_welch(table, ctypes.byref(params) if params is not None else None, int(length),
                                   ctypes.byref(stft) if stft is not None else None, flags,
                                   ctypes.byref(psd) if psd is not None else None, buf, len(buf)))
    return buf.value.decode()


def describe_csd(csd):
    """One line naming the form (two or four chains), the plan and the kernels of a cross-spectra call (bhw_describe_csd) for the
    descriptor `csd` (a BhwCsd, make_csd).  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().bhw_describe_csd(ctypes.byref(csd), buf, len(buf)))
    return buf.value.decode()


FFT_MIN_N, FFT_MAX_N = 16, 4096          # n_fft of the fused window + FFT calls: a power of two in this range


def fft_supported(n_fft):
    """True where bhw_stft_fft_f32_* take n_fft: a power of two in 16..4096."""
    n_fft = int(n_fft)
    return FFT_MIN_N <= n_fft <= FFT_MAX_N and n_fft & (n_fft - 1) == 0


def describe_stft_fft(params, length, stft, *, detrend=False, table=None):
    """One line: the route, the plan (lanes per row, rows per workgroup, radix schedule, LDS, grid) and the kernel of a fused window +
    FFT call over the window of `length`, for the descriptor `stft` (a BhwStft, make_stft; its y strides count floats of spectrum
    rows) (bhw_describe_stft_fft).  `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(768)
    check(lib().bhw_describe_stft_fft(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                      WELCH_DETREND_CONSTANT if detrend else 0, buf, len(buf)))
    return buf.value.decode()


def describe_istft_fft(params, length, stft, *, normalize=False, table=None):
    """One line: the route, the kernel and the plan (radix schedule, lanes per row, spans per workgroup, span length S, halo, share of
    repeated transforms, grid, LDS) of a fused inverse FFT + overlap-add over the window of `length`, for the descriptor `stft` (a
    BhwStft, make_stft; its y strides count floats of spectrum rows) (bhw_describe_istft_fft).  `table` is a resident table handle or
    None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().bhw_describe_istft_fft(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                       OLA_NORMALIZE if normalize else 0, buf, len(buf)))
    return buf.value.decode()


MASK_FFT_MAX_N = 2048


def mask_fft_supported(n_fft):
    """True for the n_fft the fused STFT + mask + inverse STFT kernel takes: a power of two in FFT_MIN_N..MASK_FFT_MAX_N."""
    return fft_supported(n_fft) and int(n_fft) <= MASK_FFT_MAX_N


def describe_mask_fft(params, length, analysis, synthesis, *, normalize=False, g_stride=0, g_batch_stride=0, table=None):
    """One line: the route, the kernel and the plan of a fused STFT + mask + inverse STFT call over the window of `length`
    (bhw_describe_mask_fft): the plan fields of describe_istft_fft for `synthesis` in the same words (only the LDS bytes differ),
    "forward + inverse FFT", the padding of `analysis` and the gain strides (0: one gain row for every frame / every signal).  Both
    descriptors are BhwStft (make_stft) with zero y strides.  `table` is a resident table handle or None for the library call.  Host
    arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    check(lib().bhw_describe_mask_fft(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                      OLA_NORMALIZE if normalize else 0, int(g_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


MASK_MFFT_MAX_N = 2047


def mask_mfft_supported(n_fft):
    """True for the n_fft the mixed-radix fused STFT + mask + inverse STFT kernel takes: the mfft_supported() lengths below 2048 (an
    even 2^a 3^b 5^c that is no power of two, 18..2000)."""
    return mfft_supported(n_fft) and int(n_fft) <= MASK_MFFT_MAX_N


def describe_mask_mfft(params, length, analysis, synthesis, *, normalize=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_mask_fft() for a mixed-radix n_fft (bhw_describe_mask_mfft): the plan fields of describe_istft_mfft for `synthesis` in
    the same words (only the LDS bytes differ), "forward + inverse FFT", the padding of `analysis` and the gain strides.  Host
    arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    check(lib().bhw_describe_mask_mfft(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                       OLA_NORMALIZE if normalize else 0, int(g_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


def describe_cmask_fft(params, length, analysis, synthesis, *, normalize=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_mask_fft() for the complex-gain call (bhw_describe_cmask_fft): the same plan fields -- the plan IS the real-gain
    call's; the gains live in registers -- in a line that begins "cmask", names k_cmask_fft_direct / k_cmask_fft_table and says
    "complex gains".  The gain strides count (gr, gi) pairs.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    check(lib().bhw_describe_cmask_fft(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                       OLA_NORMALIZE if normalize else 0, int(g_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


def describe_cmask_mfft(params, length, analysis, synthesis, *, normalize=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_cmask_fft() for a mixed-radix n_fft (bhw_describe_cmask_mfft): describe_mask_mfft()'s plan fields, k_cmask_mfft_direct /
    k_cmask_mfft_table and "complex gains", the strides in pairs.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    check(lib().bhw_describe_cmask_mfft(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                        OLA_NORMALIZE if normalize else 0, int(g_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


def _describe_mask_iq(name, params, length, analysis, synthesis, normalize, fftshift, g_stride, g_batch_stride, table):
    buf = ctypes.create_string_buffer(1280)
    flags = (OLA_NORMALIZE if normalize else 0) | (CFFT_SHIFT if fftshift else 0)
    check(getattr(lib(), "bhw_describe_" + name)(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                                 flags, int(g_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


def describe_mask_cfft(params, length, analysis, synthesis, *, normalize=False, fftshift=False, g_stride=0, g_batch_stride=0, table=None):
    """One line: the route, the kernel and the plan of a fused STFT + gain + inverse STFT call for I/Q input (bhw_describe_mask_cfft):
    the plan fields of describe_istft_cfft for `synthesis` in the same words (only the LDS bytes differ), with the kernel name,
    "forward + inverse FFT", the analysis padding, the gain strides and whether the gain columns are shifted.  Host arithmetic only."""
    return _describe_mask_iq("mask_cfft", params, length, analysis, synthesis, normalize, fftshift, g_stride, g_batch_stride, table)


def describe_cmask_cfft(params, length, analysis, synthesis, *, normalize=False, fftshift=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_mask_cfft() for the complex-gain call (bhw_describe_cmask_cfft): "cmask", k_cmask_cfft_*, "complex gains", strides in pairs."""
    return _describe_mask_iq("cmask_cfft", params, length, analysis, synthesis, normalize, fftshift, g_stride, g_batch_stride, table)


def describe_mask_cmfft(params, length, analysis, synthesis, *, normalize=False, fftshift=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_mask_cfft() for a mixed-radix n_fft (bhw_describe_mask_cmfft): the plan fields of describe_istft_cmfft, LDS bytes included."""
    return _describe_mask_iq("mask_cmfft", params, length, analysis, synthesis, normalize, fftshift, g_stride, g_batch_stride, table)


def describe_cmask_cmfft(params, length, analysis, synthesis, *, normalize=False, fftshift=False, g_stride=0, g_batch_stride=0, table=None):
    """describe_mask_cmfft() for the complex-gain call (bhw_describe_cmask_cmfft)."""
    return _describe_mask_iq("cmask_cmfft", params, length, analysis, synthesis, normalize, fftshift, g_stride, g_batch_stride, table)


BEAM_MAX_CH = 64   # BHW_BEAM_MAX_CH


def _describe_beam(fam, params, length, analysis, synthesis, n_ch, normalize, x_ch_stride, g_stride, g_ch_stride, g_batch_stride, table):
    buf = ctypes.create_string_buffer(1280)
    check(getattr(lib(), "bhw_describe_beam_" + fam)(table, ctypes.byref(params), int(length), ctypes.byref(analysis), ctypes.byref(synthesis),
                                                     OLA_NORMALIZE if normalize else 0, int(n_ch), int(x_ch_stride), int(g_stride),
                                                     int(g_ch_stride), int(g_batch_stride), buf, len(buf)))
    return buf.value.decode()


def describe_beam_fft(params, length, analysis, synthesis, n_ch, *, normalize=False, x_ch_stride=0, g_stride=0, g_ch_stride=0,
                      g_batch_stride=0, table=None):
    """describe_cmask_fft() for the filter-and-sum call over n_ch channels (bhw_describe_beam_fft): the same plan fields for the B
    output signals -- the channel sums live in registers -- in a line that begins "beam", names k_beam_fft_direct / k_beam_fft_table
    and says "channels C" and the three gain strides (in pairs).  Host arithmetic only."""
    return _describe_beam("fft", params, length, analysis, synthesis, n_ch, normalize, x_ch_stride, g_stride, g_ch_stride, g_batch_stride, table)


def describe_beam_mfft(params, length, analysis, synthesis, n_ch, *, normalize=False, x_ch_stride=0, g_stride=0, g_ch_stride=0,
                       g_batch_stride=0, table=None):
    """describe_beam_fft() for a mixed-radix n_fft (bhw_describe_beam_mfft): describe_cmask_mfft()'s plan fields, k_beam_mfft_direct /
    k_beam_mfft_table.  Host arithmetic only."""
    return _describe_beam("mfft", params, length, analysis, synthesis, n_ch, normalize, x_ch_stride, g_stride, g_ch_stride, g_batch_stride, table)


def describe_spectrogram(params, length, stft, *, detrend=False, fbank=None, table=None):
    """One line: the plan fields of describe_stft_fft in the same words, the mode (power or bank), W, and for a bank its filters,
    weights and filters per lane, for a fused spectrogram call over the window of `length` with the descriptor `stft` (a BhwStft,
    make_stft; its y strides count floats of output rows) and `fbank` (a BhwFbank, make_fbank, or None) (bhw_describe_spectrogram).
    `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().bhw_describe_spectrogram(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                         WELCH_DETREND_CONSTANT if detrend else 0, ctypes.byref(fbank) if fbank is not None else None,
                                         buf, len(buf)))
    return buf.value.decode()


WELCH_FFT_CHUNK = 16                     # BHW_WELCH_FFT_CHUNK: the frames of one chunk sum of the fused Welch PSD


def welch_fft_workspace_bytes(stft):
    """The bytes of workspace a fused Welch PSD call of the descriptor `stft` (a BhwStft, make_stft, y strides 0) needs: B *
    ceil(F / 16) * K chunk sums and, for F > 256, B * ceil(F / 256) * K block sums, as doubles (bhw_welch_fft_workspace_bytes)."""
    return int(lib().bhw_welch_fft_workspace_bytes(ctypes.byref(stft)))


def describe_welch_fft(params, length, stft, *, detrend=False, table=None):
    """One line: the plan fields of describe_stft_fft in the same words, plus the chunk, the runs, the groups per run, the
    accumulators per lane and the workspace bytes of a fused Welch PSD call over the window of `length` with the descriptor `stft`
    (a BhwStft, make_stft, y strides 0) (bhw_describe_welch_fft).  `table` is a resident table handle or None for the library
    call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    check(lib().bhw_describe_welch_fft(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                       WELCH_DETREND_CONSTANT if detrend else 0, buf, len(buf)))
    return buf.value.decode()


def csd_fft_workspace_bytes(stft):
    """The bytes of workspace a fused cross-spectra call of the descriptor `stft` (a BhwStft, make_stft, y strides 0) needs: four times
    welch_fft_workspace_bytes(stft), the chunk and block sums of the four chains (bhw_csd_fft_workspace_bytes)."""
    return int(lib().bhw_csd_fft_workspace_bytes(ctypes.byref(stft)))


def describe_csd_fft(params, length, stft, *, detrend=False, outputs=("pxy",), onesided=True, broadcast_x=False, table=None):
    """One line: the plan fields of describe_welch_fft in the same words for the pair plan of a fused cross-spectra call (frames of x
    and of y side by side, at most 128 lanes per row), plus the frame pairs per group, the outputs and the chains, over the window of
    `length` with the descriptor `stft` (a BhwStft, make_stft, y strides 0) (bhw_describe_csd_fft).  `table` is a resident table
    handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1536)
    flags = csd_mask(outputs) | (CSD_ONESIDED if onesided else 0) | (CSD_BROADCAST_X if broadcast_x else 0)
    check(lib().bhw_describe_csd_fft(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                     WELCH_DETREND_CONSTANT if detrend else 0, flags, buf, len(buf)))
    return buf.value.decode()


MFFT_MIN_N, MFFT_MAX_N = 16, 4095         # n_fft of the mixed-radix fused calls: even 2^a 3^b 5^c in this range, no power of two
MFFT_POWER = 2                           # BHW_MFFT_POWER


def mfft_supported(n_fft):
    """True where bhw_stft_mfft_f32_* take n_fft: even, 2^a * 3^b * 5^c, in 16..4095, and not a power of two (those go to
    bhw_stft_fft_f32_*: fft_supported)."""
    n = int(n_fft)
    if not MFFT_MIN_N <= n <= MFFT_MAX_N or n % 2 or n & (n - 1) == 0:
        return False
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def describe_stft_mfft(params, length, stft, *, detrend=False, power=False, fbank=None, table=None):
    """One line: the plan fields of describe_stft_fft in the same words for the mixed-radix transform (the schedule of radix-5, -3, -4
    and -2 passes), the output form (spectrum rows, power rows, or bank rows with the filters, weights and filters per lane) and the
    kernel, for a call over the window of `length` with the descriptor `stft` (a BhwStft, make_stft; its y strides count floats of
    output rows) and `fbank` (a BhwFbank, make_fbank, or None; it needs power=True) (bhw_describe_stft_mfft).  `table` is a resident
    table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (MFFT_POWER if power else 0)
    check(lib().bhw_describe_stft_mfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags,
                                       ctypes.byref(fbank) if fbank is not None else None, buf, len(buf)))
    return buf.value.decode()


def _describe_logspec(fn, params, length, stft, logspec, detrend, fbank, table):
    buf = ctypes.create_string_buffer(1280)
    check(fn(table, ctypes.byref(params), int(length), ctypes.byref(stft), WELCH_DETREND_CONSTANT if detrend else 0,
             ctypes.byref(fbank) if fbank is not None else None, ctypes.byref(logspec) if logspec is not None else None, buf, len(buf)))
    return buf.value.decode()


def describe_logspec(params, length, stft, logspec, *, detrend=False, fbank=None, table=None):
    """One line: the plan fields of describe_spectrogram's line in the same words, plus the rows that are logged (power or bank), the
    log stage (clamp or add, floor, mult), the DCT's shape and W, for a fused log-spectrogram / MFCC call over the window of `length`
    with the descriptor `stft` (a BhwStft; its y strides count floats of output rows), `logspec` (a BhwLogspec, make_logspec) and
    `fbank` (a BhwFbank or None) (bhw_describe_logspec).  `table` is a resident table handle or None.  Host arithmetic only."""
    return _describe_logspec(lib().bhw_describe_logspec, params, length, stft, logspec, detrend, fbank, table)


def describe_logspec_mfft(params, length, stft, logspec, *, detrend=False, fbank=None, table=None):
    """describe_logspec for the mixed-radix n_fft of describe_stft_mfft (bhw_describe_logspec_mfft): the plan fields of that call's
    line under power=True."""
    return _describe_logspec(lib().bhw_describe_logspec_mfft, params, length, stft, logspec, detrend, fbank, table)


def describe_istft_mfft(params, length, stft, *, normalize=False, table=None):
    """One line: the plan fields of describe_istft_fft in the same words for the inverse mixed-radix transform (the schedule of
    radix-5, -3, -4 and -2 passes behind the pre-split), for a fused inverse FFT + overlap-add over the window of `length` with the
    descriptor `stft` (a BhwStft, make_stft; its y strides count floats of spectrum rows) (bhw_describe_istft_mfft).  `table` is a
    resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().bhw_describe_istft_mfft(table, ctypes.byref(params), int(length), ctypes.byref(stft),
                                        OLA_NORMALIZE if normalize else 0, buf, len(buf)))
    return buf.value.decode()


CFFT_MIN_N, CFFT_MAX_N = 16, 2048        # n_fft of the fused window + complex FFT calls (I/Q input): a power of two in this range
CFFT_POWER, CFFT_SHIFT = 2, 4            # BHW_CFFT_POWER, BHW_CFFT_SHIFT


def cfft_supported(n_fft):
    """True where bhw_stft_cfft_f32_* take n_fft: a power of two in 16..2048."""
    n_fft = int(n_fft)
    return CFFT_MIN_N <= n_fft <= CFFT_MAX_N and n_fft & (n_fft - 1) == 0


def describe_stft_cfft(params, length, stft, *, detrend=False, power=False, fftshift=False, table=None):
    """One line: the plan fields of describe_stft_fft in the same words for the complex transform of I/Q rows (no split pass), the
    output form (spectrum or power rows), whether the bins are shifted, and the kernel, for a fused window + complex FFT call over
    the window of `length` with the descriptor `stft` (a BhwStft with channels 2; its y strides count floats of output rows)
    (bhw_describe_stft_cfft).  `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_POWER if power else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_stft_cfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


CMFFT_MIN_N, CMFFT_MAX_N = 16, 2047      # n_fft of the mixed-radix I/Q calls: 2^a 3^b 5^c in this range, odd or even, no power of two


def cmfft_supported(n_fft):
    """True where bhw_stft_cmfft_f32_* take n_fft: 2^a 3^b 5^c in 16..2047 that is no power of two (91 sizes, 18 of them odd)."""
    n = int(n_fft)
    if not CMFFT_MIN_N <= n <= CMFFT_MAX_N or n & (n - 1) == 0:
        return False
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def describe_stft_cmfft(params, length, stft, *, detrend=False, power=False, fftshift=False, table=None):
    """One line: the plan fields of describe_stft_cfft in the same words for the mixed-radix complex transform of I/Q rows (the
    schedule of radix-5, -3, -4 and -2 passes over n_fft points, no split pass), the entries of the twiddle table, the output form,
    whether the bins are shifted, and the kernel (bhw_describe_stft_cmfft).  `stft` is a BhwStft with channels 2; `table` is a
    resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_POWER if power else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_stft_cmfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


def describe_istft_cfft(params, length, stft, *, normalize=False, fftshift=False, table=None):
    """One line: the plan fields of describe_istft_fft in the same words for the inverse complex transform of I/Q rows (no split
    pass), whether the bins are shifted, and the kernel, for a fused inverse complex FFT + overlap-add over the window of `length`
    with the descriptor `stft` (a BhwStft with channels 2; its y strides count floats of spectrum rows) (bhw_describe_istft_cfft).
    `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    flags = (OLA_NORMALIZE if normalize else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_istft_cfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


def describe_istft_cmfft(params, length, stft, *, normalize=False, fftshift=False, table=None):
    """One line: the plan fields of describe_istft_cfft in the same words for the inverse mixed-radix complex transform of I/Q rows
    (the schedule of radix-5, -3, -4 and -2 passes over n_fft points, no split pass), the entries of the twiddle table, whether the
    bins are shifted, and the kernel (bhw_describe_istft_cmfft).  `stft` is a BhwStft with channels 2 whose y strides count floats of
    spectrum rows; `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1024)
    flags = (OLA_NORMALIZE if normalize else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_istft_cmfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


def welch_cfft_workspace_bytes(stft):
    """The bytes of workspace a fused Welch PSD call for I/Q input of the descriptor `stft` (a BhwStft with channels 2, y strides 0)
    needs: B * ceil(F / 16) * n_fft chunk sums and, for F > 256, B * ceil(F / 256) * n_fft block sums, as doubles
    (bhw_welch_cfft_workspace_bytes)."""
    return int(lib().bhw_welch_cfft_workspace_bytes(ctypes.byref(stft)))


def describe_welch_cfft(params, length, stft, *, detrend=False, fftshift=False, table=None):
    """One line: the plan fields of describe_stft_cfft in the same words (without the output form), plus the chunk, the runs, the
    groups per run, the accumulators per lane and the workspace bytes of a fused Welch PSD call for I/Q input over the window of
    `length` with the descriptor `stft` (a BhwStft with channels 2, y strides 0) (bhw_describe_welch_cfft).  `table` is a resident
    table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_welch_cfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


def welch_mfft_workspace_bytes(stft):
    """The bytes of workspace a fused Welch PSD call at a mixed-radix n_fft of the descriptor `stft` (a BhwStft with channels 1,
    y strides 0) needs: B * ceil(F / 16) * K chunk sums, K = n_fft / 2 + 1, and, for F > 256, B * ceil(F / 256) * K block sums, as
    doubles (bhw_welch_mfft_workspace_bytes)."""
    return int(lib().bhw_welch_mfft_workspace_bytes(ctypes.byref(stft)))


def describe_welch_mfft(params, length, stft, *, detrend=False, table=None):
    """One line: the plan fields of describe_stft_mfft in the same words (without the output form), plus the chunk, the runs, the
    groups per run, the accumulators per lane and the workspace bytes of a fused Welch PSD call at a mixed-radix n_fft over the
    window of `length` with the descriptor `stft` (a BhwStft with channels 1, y strides 0) (bhw_describe_welch_mfft).  `table` is a
    resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    flags = WELCH_DETREND_CONSTANT if detrend else 0
    check(lib().bhw_describe_welch_mfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


def welch_cmfft_workspace_bytes(stft):
    """The bytes of workspace a fused Welch PSD call for I/Q input at a mixed-radix n_fft of the descriptor `stft` (a BhwStft with
    channels 2, y strides 0) needs: B * ceil(F / 16) * n_fft chunk sums and, for F > 256, B * ceil(F / 256) * n_fft block sums, as
    doubles (bhw_welch_cmfft_workspace_bytes)."""
    return int(lib().bhw_welch_cmfft_workspace_bytes(ctypes.byref(stft)))


def describe_welch_cmfft(params, length, stft, *, detrend=False, fftshift=False, table=None):
    """One line: the plan fields of describe_stft_cmfft in the same words (without the output form), plus the chunk, the runs, the
    groups per run, the accumulators per lane and the workspace bytes of a fused Welch PSD call for I/Q input at a mixed-radix n_fft
    over the window of `length` with the descriptor `stft` (a BhwStft with channels 2, y strides 0) (bhw_describe_welch_cmfft).
    `table` is a resident table handle or None for the library call.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_welch_cmfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, buf, len(buf)))
    return buf.value.decode()


HOLD_MAX, HOLD_MIN = 1, 2
_HOLD_TRACES = {"both": HOLD_MAX | HOLD_MIN, "max": HOLD_MAX, "min": HOLD_MIN}


def hold_traces(traces):
    """The trace mask of the hold calls from "both" | "max" | "min" (ValueError otherwise)."""
    try:
        return _HOLD_TRACES[traces]
    except (KeyError, TypeError):
        raise ValueError(f"traces must be 'both', 'max' or 'min', got {traces!r}") from None


def hold_cfft_workspace_bytes(stft):
    """The bytes of workspace a fused max-hold / min-hold call for I/Q input of the descriptor `stft` (a BhwStft with channels 2,
    y strides 0) needs: welch_cfft_workspace_bytes(stft) -- a (max, min) pair of float32 words per chunk and block takes the 8 bytes
    of a chunk sum (bhw_hold_cfft_workspace_bytes)."""
    return int(lib().bhw_hold_cfft_workspace_bytes(ctypes.byref(stft)))


def describe_hold_cfft(params, length, stft, *, detrend=False, fftshift=False, traces="both", table=None):
    """One line: the fields of describe_welch_cfft in the same words ("hold cfft ...", with the hold kernels and their join), plus
    the traces that are stored ("both" | "max" | "min"), for a fused max-hold / min-hold call for I/Q input over the window of
    `length` with the descriptor `stft` (bhw_describe_hold_cfft).  `table` is a resident table handle or None for the library call.
    Host arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_hold_cfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, hold_traces(traces), buf,
                                       len(buf)))
    return buf.value.decode()


def hold_cmfft_workspace_bytes(stft):
    """hold_cfft_workspace_bytes() at a mixed-radix n_fft: welch_cmfft_workspace_bytes(stft) (bhw_hold_cmfft_workspace_bytes)."""
    return int(lib().bhw_hold_cmfft_workspace_bytes(ctypes.byref(stft)))


def describe_hold_cmfft(params, length, stft, *, detrend=False, fftshift=False, traces="both", table=None):
    """describe_hold_cfft() at a mixed-radix n_fft: the fields of describe_welch_cmfft in the same words ("hold cmfft ..."), plus
    the traces that are stored (bhw_describe_hold_cmfft)."""
    buf = ctypes.create_string_buffer(1280)
    flags = (WELCH_DETREND_CONSTANT if detrend else 0) | (CFFT_SHIFT if fftshift else 0)
    check(lib().bhw_describe_hold_cmfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, hold_traces(traces), buf,
                                        len(buf)))
    return buf.value.decode()


def hold_fft_workspace_bytes(stft):
    """The bytes of workspace a fused max-hold / min-hold call for real input of the descriptor `stft` (a BhwStft with channels 1,
    y strides 0) needs: welch_fft_workspace_bytes(stft) -- a (max, min) pair of float32 words per chunk and block takes the 8 bytes
    of a chunk sum (bhw_hold_fft_workspace_bytes)."""
    return int(lib().bhw_hold_fft_workspace_bytes(ctypes.byref(stft)))


def describe_hold_fft(params, length, stft, *, detrend=False, traces="both", table=None):
    """One line: the fields of describe_welch_fft in the same words ("hold fft ...", with the hold kernels and their join), plus the
    traces that are stored ("both" | "max" | "min"), for a fused max-hold / min-hold call for real input over the window of `length`
    with the descriptor `stft` (bhw_describe_hold_fft).  `table` is a resident table handle or None for the library call.  Host
    arithmetic only."""
    buf = ctypes.create_string_buffer(1280)
    flags = WELCH_DETREND_CONSTANT if detrend else 0
    check(lib().bhw_describe_hold_fft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, hold_traces(traces), buf,
                                      len(buf)))
    return buf.value.decode()


def hold_mfft_workspace_bytes(stft):
    """hold_fft_workspace_bytes() at a mixed-radix n_fft: welch_mfft_workspace_bytes(stft) (bhw_hold_mfft_workspace_bytes)."""
    return int(lib().bhw_hold_mfft_workspace_bytes(ctypes.byref(stft)))


def describe_hold_mfft(params, length, stft, *, detrend=False, traces="both", table=None):
    """describe_hold_fft() at a mixed-radix n_fft: the fields of describe_welch_mfft in the same words ("hold mfft ..."), plus the
    traces that are stored (bhw_describe_hold_mfft)."""
    buf = ctypes.create_string_buffer(1280)
    flags = WELCH_DETREND_CONSTANT if detrend else 0
    check(lib().bhw_describe_hold_mfft(table, ctypes.byref(params), int(length), ctypes.byref(stft), flags, hold_traces(traces), buf,
                                       len(buf)))
    return buf.value.decode()


def sums_from_words(words, shift, length):
    """The window sums from the four result words of bhw_window_sums_*: (s1, s2) as Python ints, S1 = s1 * 2^-shift and
    S2 = s2 * 2^-2 shift each rounded once to a float, coherent_gain = S1 / L and enbw_bins = L * S2 / S1^2."""
    from fractions import Fraction
    s1 = int(words[0]) - (1 << 64) if int(words[0]) >> 63 else int(words[0])
    s2 = int(words[1]) + (int(words[2]) << 32)
    if int(words[3]) != int(length):
        raise RuntimeError(f"window sums counted {int(words[3])} coefficients, expected {int(length)}")
    S1, S2 = float(Fraction(s1, 1 << shift)), float(Fraction(s2, 1 << (2 * shift)))
    return {"s1": s1, "s2": s2, "S1": S1, "S2": S2, "length": int(length), "shift": int(shift),
            "coherent_gain": S1 / length, "enbw_bins": length * S2 / (S1 * S1) if s1 else float("inf")}


def welch_scale(sums, frames, fs=1.0, scaling="density"):
    """The periodogram scale of scipy.signal.welch from the window sums: 1 / (fs * S2 * F) (density) or 1 / (S1^2 * F) (spectrum)."""
    if scaling == "density":
        return 1.0 / (float(fs) * sums["S2"] * frames)
    if scaling == "spectrum":
        return 1.0 / (sums["S1"] * sums["S1"] * frames)
    raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")


def part_segments(params, part, n_parts):
    """[(n0, count), ...]: the coefficients interleaved-ownership part `part` of `n_parts` owns (bhw_part_segments).  Host arithmetic."""
    n = ctypes.c_uint32()
    segs = (BhwSegment * 256)()
    check(lib().bhw_part_segments(ctypes.byref(params), part, n_parts, segs, 256, ctypes.byref(n)))
    return [(int(segs[i].n0), int(segs[i].count)) for i in range(n.value)]


def coeffs_from_float(win_type, dat_width, a=None):
    """a_k = round(coe_k * (2^(W-s) - 1)) -- hls/windows/win_function.cpp:176-177,...,349-355."""
    aa = (ctypes.c_int32 * 7)()
    arr = None
    if a is not None:
        arr = (ctypes.c_double * 7)(*(list(a) + [0.0] * (7 - len(a))))
    check(lib().bhw_coeffs_from_float(win_type, dat_width, arr, aa))
    return list(aa)


PRESETS = {"nuttall": 1, "blackman-nuttall": 2, "flat-top-1": 3, "flat-top-2": 4, "bh7-readme": 5, "blackman": 6, "bh3": 7}


def coeffs_preset(name, dat_width):
    """(win_type, float weights, integer weights) of a named coefficient set the reference lists beside its built-ins
    (bhw_coeffs_preset: hls/windows/win_function.cpp:241-250,292-303, README.md:30-51)."""
    wt = ctypes.c_uint32(0)
    a = (ctypes.c_double * 7)()
    aa = (ctypes.c_int32 * 7)()
    check(lib().bhw_coeffs_preset(PRESETS[name] if isinstance(name, str) else int(name), dat_width, ctypes.byref(wt), a, aa))
    return int(wt.value), list(a), list(aa)


def constant_tables(which):
    t = (ctypes.c_int64 * 48)()
    g = (ctypes.c_int64 * 2)()
    check(lib().bhw_constant_tables(which, t, g))
    return list(t), list(g)


def make_params(win_type, phi_width, dat_width, *, model=MODEL_HLS, combine=COMBINE_HLS, sin_type=SIN_CORDIC,
                precision=1, lut_size=9, aa=None, n_terms=None, validate=True):
    """Build a bhw_params.  `aa` overrides the built-in integer weights (the AA0..AA6 ports)."""
    p = BhwParams()
    rc = lib().bhw_params_init(ctypes.byref(p), win_type, phi_width, dat_width)
    # bhw_params_init validates with the defaults (model HLS); re-validate below with the caller's choices
    if rc != 0 and p.n_terms == 0:
        check(rc)
    p.model, p.combine, p.sin_type = model, combine, sin_type
    p.precision, p.lut_size = precision, lut_size
    if n_terms is not None:
        p.n_terms = n_terms
    if aa is not None:
        vals = list(aa) + [0] * (7 - len(aa))
        for k in range(7):
            p.aa[k] = int(vals[k])
    # the variant generators (cordic_dds48 / cordic_dds_scaled) are sin/cos sources only: bhw_sincos_* validates them
    if validate and model <= MODEL_VHDL:
        check(lib().bhw_params_validate(ctypes.byref(p)))
    return p
