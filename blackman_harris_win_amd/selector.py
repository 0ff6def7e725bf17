"""Host-side mirror of the reference's operator interface, on top of the C ABI.

torch is plumbing here: it owns the output tensor, the current stream and (in bench.py) the
process group.  The arithmetic is in libbhw.so's HIP kernels.
"""
import ctypes
import math

from . import binding as B

_WIN_TYPES = {
    # WIN_TYPE generic strings of win_selector (src/win_selector.vhd:64,93,115,137,157,178) plus the
    # HLS names (hls/windows/window_test.cpp:59-74)
    "HAMMING": B.WIN_HAMMING, "HANN": B.WIN_HANN,
    "BH3TERM": B.WIN_BH3, "BH4TERM": B.WIN_BH4, "BH5TERM": B.WIN_BH5, "BH7TERM": B.WIN_BH7,
    "Hamming": B.WIN_HAMMING, "Hann": B.WIN_HANN, "Blackman-Harris-3": B.WIN_BH3,
    "Blackman-Harris-4": B.WIN_BH4, "Blackman-Harris-5": B.WIN_BH5, "Blackman-Harris-7": B.WIN_BH7,
}


_TORCH = None


def _torch():
    """torch, once a HIP device has been seen (cached: the per-call cost of the wrappers matters for short windows)."""
    global _TORCH
    if _TORCH is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the window generator runs only on the GPU (no CPU fallback)")
        _TORCH = torch
    return _TORCH


def _stream_ptr(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev_index(torch, device):
    d = torch.device("cuda" if device is None else device)
    return torch.cuda.current_device() if d.index is None else d.index


def shard_range(total, rank, world_size):
    """Contiguous index shard [n0, n0+count) of `total` coefficients for `rank` (no collective)."""
    base, rem = divmod(total, world_size)
    n0 = rank * base + min(rank, rem)
    return n0, base + (1 if rank < rem else 0)


def _check_out(torch, out, need, what="out", dtype=None):
    """An output tensor handed to the kernels: int32 (or `dtype`), on a GPU, contiguous, large enough."""
    dtype = torch.int32 if dtype is None else dtype
    if out.dtype != dtype or not out.is_cuda or not out.is_contiguous() or out.numel() < need:
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} CUDA tensor with at least {need} elements")
    return out.device.index


def _exec(algo, workspace, event_after_build=None, table_format=B.TABLE_BEST):
    ex = B.BhwExec()
    ex.struct_size = ctypes.sizeof(B.BhwExec)
    ex.algo = algo
    ex.table_format = table_format
    if workspace is not None:
        if not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError("workspace must be a contiguous CUDA tensor")
        ex.workspace = workspace.data_ptr()
        ex.workspace_bytes = workspace.numel() * workspace.element_size()
    if event_after_build is not None:      # a torch.cuda.Event that has been recorded once (its handle exists)
        ex.event_after_build = event_after_build.cuda_event
    return ex


def prepare(params, *, device=None):
    """Every lazy step of later calls with `params` on the current stream, done now (bhw_prepare_device): Taylor ROM upload,
    library scratch, one-off verification of the packed table formats.  Needed before capturing calls into a HIP graph
    without a caller workspace; otherwise optional."""
    torch = _torch()
    dev = _dev_index(torch, device)
    B.check(B.lib().bhw_prepare_device(ctypes.byref(params), dev, _stream_ptr(torch, dev)))


def generate(params, n0, count, *, device=None, out=None, algo=B.ALGO_AUTO, workspace=None, event_after_build=None,
             table_format=B.TABLE_BEST, length=None):
    """count coefficients starting at stream index n0 as an int32 CUDA tensor (bhw_generate_device).  length: the window length L
    (1..2^phi_width) of a window of any length (bhw_generate_len_device; algo, workspace, event_after_build and table_format do not
    apply); None: the power-of-two window, N = 2^phi_width."""
    torch = _torch()
    dev = _dev_index(torch, device)
    if out is None:
        out = torch.empty(int(count), dtype=torch.int32, device=f"cuda:{dev}")
    else:
        dev = _check_out(torch, out, int(count))
    ex = ()
    if length is None:
        if workspace is not None and workspace.device.index != dev:
            raise ValueError("workspace must live on the output's device")
        ex = (ctypes.byref(_exec(algo, workspace, event_after_build, table_format)),)
    _call("bhw_generate_device_ex", "bhw_generate_len_device", (), params, length,
          (dev, _stream_ptr(torch, dev), int(n0), int(count), ctypes.c_void_p(out.data_ptr())), ex)
    return out


def generate_part(params, part, n_parts, window, *, algo=B.ALGO_AUTO, workspace=None, event_after_build=None,
                  table_format=B.TABLE_BEST):
    """Interleaved ownership (bhw_generate_part_device): writes the coefficients part `part` of `n_parts` owns into `window`,
    a full-length (2^phi_width) int32 CUDA tensor; every other element is left untouched.  binding.part_segments lists them."""
    torch = _torch()
    dev = _check_out(torch, window, 1 << params.phi_width, "window")
    if workspace is not None and workspace.device.index != dev:
        raise ValueError("workspace must live on the window's device")
    ex = _exec(algo, workspace, event_after_build, table_format)
    B.check(B.lib().bhw_generate_part_device(ctypes.byref(params), dev, _stream_ptr(torch, dev), int(part), int(n_parts),
                                              ctypes.c_void_p(window.data_ptr()), ctypes.byref(ex)))
    return window


def gather_parts(params, windows, out):
    """One window on out's device from its interleaved ownership parts (bhw_gather_parts_device): windows[g] is the full-length
    int32 CUDA tensor part g of len(windows) was generated into (any device; windows[g] may be `out` itself).  Peer copies of the
    owned segments on out's current stream; the producing streams must have been synchronised with it by the caller."""
    torch = _torch()
    n = 1 << params.phi_width
    dev = _check_out(torch, out, n)
    G = len(windows)
    devs = (ctypes.c_int * G)(*[_check_out(torch, w, n, "window") for w in windows])
    ptrs = (ctypes.c_void_p * G)(*[w.data_ptr() for w in windows])
    B.check(B.lib().bhw_gather_parts_device(ctypes.byref(params), G, devs, ptrs, dev, _stream_ptr(torch, dev),
                                             ctypes.c_void_p(out.data_ptr())))
    return out


def apply(params, x, *, n0=0, shift=None, out=None):
    """Fused apply: y[i] = (x[i] * w[n0+i]) >> shift without materialising w (bhw_apply_device).
    `shift` defaults to dat_width - 1 (unit gain for a full-scale window)."""
    torch = _torch()
    if x.dtype != torch.int32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous int32 CUDA tensor")
    dev = x.device.index
    if out is None:
        out = torch.empty_like(x)
    elif _check_out(torch, out, x.numel()) != dev:
        raise ValueError("out must live on x's device")
    if shift is None:
        shift = params.dat_width - 1
    B.check(B.lib().bhw_apply_device(ctypes.byref(params), dev, _stream_ptr(torch, dev), int(n0), x.numel(),
                                      ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), int(shift)))
    return out


def _call(pow2, any_len, lead, params, length, args, pow2_args=()):
    """One C call of a front: pow2(*lead, params, *args, *pow2_args) for the power-of-two window (length None), else its
    any-length entry point any_len(*lead, params, length, *args)."""
    if length is None:
        B.check(getattr(B.lib(), pow2)(*lead, ctypes.byref(params), *args, *pow2_args))
    else:
        B.check(getattr(B.lib(), any_len)(*lead, ctypes.byref(params), int(length), *args))


def _window_len(params, length):
    """N: 2^phi_width, or the window length L of a call for a window of any length."""
    return (1 << params.phi_width) if length is None else int(length)


def window(params, length, *, sym=False, device=None, out=None, dtype=None, shift=None):
    """The int32 coefficients of the window of length `length` (1..2^phi_width): the periodic (DFT-even, spectral-analysis) window
    bhw_generate_len_device(length, n0 = 0, count = length), or with sym=True the symmetric (filter-design) window: the periodic
    window of length - 1 plus its first coefficient (length >= 2).
    dtype=torch.float32: the float coefficients v = fl32(w) * 2^-shift the float32 frames and overlap-add calls apply (shift
    defaults to dat_width - 1), e.g. the window of torch.stft / torch.istft; `out` is then not taken."""
    length = int(length)
    if sym and length < 2:
        raise ValueError("a symmetric window needs length >= 2")
    torch = _torch() if dtype is not None else None
    if dtype is not None and dtype not in (torch.int32, torch.float32):
        raise ValueError("dtype must be torch.int32 or torch.float32")
    if dtype is not None and dtype == torch.float32:
        if out is not None:
            raise ValueError("out is taken for the int32 window only")
        return _float_window(torch, window(params, length, sym=sym, device=device), params, shift)
    if shift is not None:
        raise ValueError("shift applies to the float32 window only")
    return generate(params, 0, length, device=device, out=out, length=length - 1 if sym else length)


def _float_window(torch, w, params, shift):
    """v = fl32(w) * 2^-shift: the int32 window to binary32 (round to nearest even), then an exact power-of-two scaling."""
    shift = params.dat_width - 1 if shift is None else int(shift)
    if not 0 <= shift <= 62:
        raise ValueError("shift must be in 0..62")
    return w.to(torch.float32) * 2.0 ** -shift                  # 2^-shift is a binary32 power of two: the product is exact


def _frames_call(torch, params, x, hop, frames, channels, shift, out, y_stride, dev, length=None):
    """Checks and shapes of apply_frames: (bhw_frames, out, the tensor returned); y takes x's dtype (int32 or float32)."""
    if x.dtype not in (torch.int32, torch.float32) or not x.is_cuda or not x.is_contiguous() or x.device.index != dev:
        raise ValueError("x must be a contiguous int32 or float32 CUDA tensor on the call's device")
    if channels not in (1, 2):
        raise ValueError("channels must be 1 or 2")
    if hop < 1:
        raise ValueError("hop must be >= 1")
    N = _window_len(params, length)
    samples = x.numel() // channels
    if x.numel() % channels:
        raise ValueError("x must hold whole I/Q pairs")
    if frames is None:
        frames = 0 if samples < N else (samples - N) // hop + 1
    if frames and ((frames - 1) * hop + N) > samples:
        raise ValueError(f"x holds {samples} time indices, {frames} frames at hop {hop} need {(frames - 1) * hop + N}")
    stride = N * channels if y_stride is None else int(y_stride)
    if stride < N * channels:
        raise ValueError(f"y_stride must be >= N * channels = {N * channels}")
    if out is None:
        out = torch.empty((frames, stride), dtype=x.dtype, device=x.device)
    elif _check_out(torch, out, frames * stride if frames else 0, dtype=x.dtype) != dev:
        raise ValueError("out must live on x's device")
    if shift is None:
        shift = params.dat_width - 1
    f = B.make_frames(frames, hop, channels=channels, shift=shift, y_stride=stride)
    flat = out.view(-1)[:frames * stride]
    if y_stride is not None:
        result = flat.view(frames, stride)
    else:
        result = flat.view((frames, N, 2) if channels == 2 else (frames, N))
    return f, out, result


def apply_frames(params, x, hop, *, frames=None, channels=1, shift=None, out=None, y_stride=None, length=None):
    """Overlapped-frame apply (bhw_apply_frames_device): y[f, k, c] = (x[(f * hop + k) * C + c] * w[k]) >> shift for every frame f,
    with one launch (the STFT / Welch front end).  x: contiguous int32 (time-major, I/Q interleaved for channels = 2); frames=None
    takes as many as fit.  Returns a (frames, N) int32 tensor, (frames, N, 2) for I/Q, or a (frames, y_stride) view when y_stride
    is given (the elements past N * channels of each row are not written).  shift defaults to dat_width - 1.  length: the window
    length L of a window of any length (bhw_apply_frames_len_device; N is L in the shapes above); None: N = 2^phi_width.
    A float32 x takes bhw_apply_frames_f32_device: y = fl32(x * v[k]) with v = window(..., dtype=torch.float32, shift=shift), in
    float32 tensors of the same shapes."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a contiguous int32 or float32 CUDA tensor")
    dev = x.device.index
    f, out, result = _frames_call(torch, params, x, int(hop), frames, channels, shift, out, y_stride, dev, length)
    args = (dev, _stream_ptr(torch, dev), ctypes.byref(f), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    if x.dtype == torch.float32:
        B.check(B.lib().bhw_apply_frames_f32_device(ctypes.byref(params), _window_len(params, length), *args))
    else:
        _call("bhw_apply_frames_device", "bhw_apply_frames_len_device", (), params, length, args)
    return result


def _ola_call(torch, params, y, hop, frames, channels, shift, out, y_stride, t0, count, dev, length=None, normalize=False):
    """Checks and shapes of overlap_add: (bhw_ola, out, the tensor returned, flags); x takes y's dtype (int32 or float32)."""
    if not isinstance(y, torch.Tensor) or y.dtype not in (torch.int32, torch.float32) or not y.is_cuda or not y.is_contiguous() \
            or y.device.index != dev:
        raise ValueError("y must be a contiguous int32 or float32 CUDA tensor on the call's device")
    if normalize and y.dtype != torch.float32:
        raise ValueError("normalize=True takes a float32 y (the int32 overlap-add has no envelope division)")
    if channels not in (1, 2):
        raise ValueError("channels must be 1 or 2")
    if hop < 1:
        raise ValueError("hop must be >= 1")
    N = _window_len(params, length)
    if y.dim() < 1:
        raise ValueError("y must be (frames, N), (frames, N, 2) or (frames, y_stride)")
    rows = y.shape[0]
    row_len = y.numel() // rows if rows else N * channels
    stride = row_len if y_stride is None else int(y_stride)
    if stride < N * channels:
        raise ValueError(f"y_stride must be >= N * channels = {N * channels}")
    if frames is None:
        frames = rows
    if frames and (frames - 1) * stride + N * channels > y.numel():
        raise ValueError(f"y holds {y.numel()} int32, {frames} frames at stride {stride} need {(frames - 1) * stride + N * channels}")
    extent = (frames - 1) * hop + N if frames else 0
    t0 = int(t0)
    if count is None:
        count = max(0, extent - t0)
    count = int(count)
    if out is None:
        out = torch.empty((count, 2) if channels == 2 else (count,), dtype=y.dtype, device=y.device)
    elif _check_out(torch, out, count * channels, dtype=y.dtype) != dev:
        raise ValueError("out must live on y's device")
    if shift is None:
        shift = params.dat_width - 1
    o = B.make_ola(frames, hop, count, t0=t0, channels=channels, shift=shift, y_stride=stride)
    result = out.view(-1)[:count * channels].view((count, 2) if channels == 2 else (count,))
    return o, out, result, (B.OLA_NORMALIZE if normalize else 0)


def overlap_add(params, y, hop, *, frames=None, channels=1, shift=None, out=None, y_stride=None, t0=0, count=None, length=None,
                normalize=False):
    """Weighted overlap-add (bhw_overlap_add_device), the STFT synthesis side in one launch:
    x[t - t0, c] = (sum over frames f of y[f, t - f * hop, c] * w[t - f * hop]) >> shift for t in [t0, t0 + count), the sum in
    int64 (wrapping), the low 32 bits stored.  y: contiguous int32 (frames, N), (frames, N, 2) for I/Q, or (frames, y_stride)
    rows of which the first N * channels are read.  frames=None takes every row; count=None the whole extent
    (frames - 1) * hop + N from t0; shift defaults to dat_width - 1.  Returns (count,) int32, or (count, 2) for I/Q.  length: the
    window length L of a window of any length (bhw_overlap_add_len_device; N is L above); None: N = 2^phi_width.
    A float32 y takes bhw_overlap_add_f32_device: the sum in binary64 over the frames in ascending order of (double) y * v[k]
    (v = window(..., dtype=torch.float32, shift=shift)), rounded to float32; normalize=True (float32 only) divides it by the window
    envelope, the sum of v[k]^2 over the same frames (+0.0 where no frame reaches t), as torch.istft does."""
    torch = _torch()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise ValueError("y must be a contiguous int32 or float32 CUDA tensor")
    dev = y.device.index
    o, out, result, flags = _ola_call(torch, params, y, int(hop), frames, channels, shift, out, y_stride, t0, count, dev, length, normalize)
    if y.dtype == torch.float32:
        B.check(B.lib().bhw_overlap_add_f32_device(ctypes.byref(params), _window_len(params, length), dev, _stream_ptr(torch, dev),
                                                   ctypes.byref(o), flags, ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(out.data_ptr())))
    else:
        _call("bhw_overlap_add_device", "bhw_overlap_add_len_device", (), params, length,
              (dev, _stream_ptr(torch, dev), ctypes.byref(o), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(out.data_ptr())))
    return result


_PAD_MODES = {"constant": B.PAD_CONSTANT, "reflect": B.PAD_REFLECT}


def _stft_window(params, n_fft, win_length):
    """(n_fft, L, col0): the window of win_length (default n_fft) centred in an n_fft row as torch.stft centres it."""
    n_fft = int(n_fft)
    L = n_fft if win_length is None else int(win_length)
    if n_fft < 1:
        raise ValueError("n_fft must be >= 1")
    if not 1 <= L <= n_fft:
        raise ValueError(f"expected 0 < win_length <= n_fft, but got win_length={L}, n_fft={n_fft}")
    if L > 1 << params.phi_width:
        raise ValueError(f"win_length {L} above 2^phi_width = {1 << params.phi_width}")
    return n_fft, L, (n_fft - L) // 2


def _stft_float(torch, t, what, dev):
    """C of a float32 (1) or complex64 (2, interleaved pairs) CUDA tensor on `dev`."""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.complex64) or not t.is_cuda or t.device.index != dev:
        raise ValueError(f"{what} must be a float32 or complex64 CUDA tensor on the call's device")
    return 2 if t.dtype == torch.complex64 else 1


def _stft_input(t, packed):
    """t as the kernels read it: its elements in memory (a lazy conjugate or negation resolved), contiguous along the last axis, and
    every outer stride at least the packed size of what it steps over (`packed`: the minimum stride per leading axis, in elements).
    Anything else -- a broadcast (stride 0), overlapping or transposed view -- is copied first: the descriptor takes 0 for packed
    and the checks cannot tell such a view from a buffer that holds the data."""
    t = t.resolve_conj().resolve_neg()
    ok = t.shape[-1] <= 1 or t.stride(-1) == 1
    for axis, need in enumerate(packed):
        ok = ok and (t.shape[axis] <= 1 or t.stride(axis) >= need)
    return t if ok else t.contiguous()


def _stft_out(torch, out, shape, like, what):
    """The output tensor: allocated, or the caller's `out` of the shape the call returns (contiguous, no lazy conjugate or negation)."""
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if not isinstance(out, torch.Tensor) or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous() \
            or out.is_conj() or out.is_neg() or tuple(out.shape) != tuple(shape):
        raise ValueError(f"out must be a contiguous {str(like.dtype).replace('torch.', '')} tensor of shape {tuple(shape)} on {what}'s device")
    return out


def _stft_frames_call(torch, params, x, n_fft, hop, win_length, center, pad_mode, shift, out, dev):
    """Checks and shapes of stft_frames: (bhw_stft, L, the x read, out)."""
    C = _stft_float(torch, x, "x", dev)
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    hop = int(hop)
    if hop < 1:
        raise ValueError("hop must be >= 1")
    n_fft, L, col0 = _stft_window(params, n_fft, win_length)
    if pad_mode not in _PAD_MODES:
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    pad = n_fft // 2 if center else 0
    if pad and pad_mode == "reflect" and pad >= T:
        raise ValueError(f"reflect padding needs pad {pad} < T = {T} (n_fft // 2 < the signal's length)")
    if nb < 1 or T + 2 * pad < n_fft:
        raise ValueError(f"zero frames: T + 2 * pad = {T + 2 * pad} < n_fft = {n_fft}" if nb else "zero signals")
    frames = 1 + (T + 2 * pad - n_fft) // hop
    xb = _stft_input(xb, (T,))
    shape = (nb, frames, n_fft) if x.dim() == 2 else (frames, n_fft)
    out = _stft_out(torch, out, shape, x, "x")
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, hop, n_fft, col0=col0, pad=pad, pad_mode=_PAD_MODES[pad_mode], channels=C, shift=shift,
                    x_stride=xb.stride(0) * C if nb > 1 else 0)
    return s, L, xb, out


def _istft_call(torch, params, y, n_fft, hop, win_length, center, length, normalize, shift, out, dev):
    """Checks and shapes of istft_overlap_add: (bhw_stft, L, the y read, out, flags)."""
    C = _stft_float(torch, y, "y", dev)
    if y.dim() not in (2, 3):
        raise ValueError("y must be (frames, n_fft) or (B, frames, n_fft)")
    hop = int(hop)
    if hop < 1:
        raise ValueError("hop must be >= 1")
    n_fft, L, col0 = _stft_window(params, n_fft, win_length)
    if not center and L < n_fft:
        raise ValueError("center=False with win_length < n_fft: the first outputs have no window under them")
    yb = y if y.dim() == 3 else y.unsqueeze(0)
    nb, frames, cols = yb.shape
    if cols != n_fft:
        raise ValueError(f"y rows hold {cols} columns, n_fft is {n_fft}")
    if frames < 1 or nb < 1:
        raise ValueError("zero frames")
    pad = n_fft // 2 if center else 0
    length = n_fft + hop * (frames - 1) - 2 * pad if length is None else int(length)
    if length < 0:
        raise ValueError(f"length {length} < 0")
    yb = _stft_input(yb, ((frames - 1) * max(yb.stride(1), n_fft) + n_fft, n_fft))
    out = _stft_out(torch, out, (nb, length) if y.dim() == 3 else (length,), y, "y")
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, length, frames, hop, n_fft, col0=col0, pad=pad, channels=C, shift=shift,
                    y_stride=yb.stride(1) * C if frames > 1 else 0, y_batch_stride=yb.stride(0) * C if nb > 1 else 0)
    return s, L, yb, out, (B.OLA_NORMALIZE if normalize else 0)


def stft_frames(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", shift=None, out=None):
    """The framing of torch.stft for a batch, in one launch (bhw_stft_frames_f32_device): x (T,) or (B, T), float32 or complex64,
    padded by n_fft // 2 on both sides (center=True; pad_mode "reflect" or "constant"), cut into frames of n_fft
    at `hop`, and the window of win_length (default n_fft; v = window(params, win_length, dtype=torch.float32, shift=shift)) applied
    in the columns [(n_fft - win_length) // 2, +win_length) of each row; the other columns are +0.0.  Returns (B, frames, n_fft), or
    (frames, n_fft) for 1-D x, in x's dtype, frames = 1 + (T + 2 * pad - n_fft) // hop.  torch.fft.rfft (fft for complex x) of the
    result, transposed to (..., n_fft // 2 + 1, frames), is torch.stft(x, n_fft, hop, win_length, window=v, center=center,
    pad_mode=pad_mode, return_complex=True).  The kernel reads x in place when its rows are contiguous and apart (x[1:, :T] of a
    wider buffer, say); a view that is not -- a broadcast (expand), transposed or lazily conjugated x -- is copied first.  `out`: a
    contiguous tensor of the returned shape."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 or complex64 CUDA tensor")
    dev = x.device.index
    s, L, xr, out = _stft_frames_call(torch, params, x, n_fft, hop, win_length, center, pad_mode, shift, out, dev)
    B.check(B.lib().bhw_stft_frames_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), ctypes.byref(s),
                                               ctypes.c_void_p(xr.data_ptr()), ctypes.c_void_p(out.data_ptr())))
    return out


def istft_overlap_add(params, y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, out=None):
    """The overlap-add of torch.istft for a batch, in one launch (bhw_istft_ola_f32_device): y (B, frames, n_fft) or (frames, n_fft),
    float32 or complex64 (e.g. torch.fft.irfft(spec.transpose(-1, -2), n=n_fft)).  Each output t < length sums,
    in ascending frame order in binary64, the frame elements under the window at padded time t + n_fft // 2 (center=True) times v
    (window(params, win_length, dtype=torch.float32, shift=shift)), and with normalize=True divides by the window envelope, the sum of
    v^2 (+0.0 where no frame reaches t).  length defaults to torch.istft's n_fft + hop * (frames - 1) - 2 * pad; outputs past the frames'
    extent are +0.0.  Returns (B, length), or (length,) for 2-D y, in y's dtype.  y is read in place when its rows and signals are
    contiguous along n_fft and apart; a broadcast, overlapping, transposed or lazily conjugated y is copied first.  `out`: a contiguous
    tensor of the returned shape."""
    torch = _torch()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise ValueError("y must be a float32 or complex64 CUDA tensor")
    dev = y.device.index
    s, L, yr, out, flags = _istft_call(torch, params, y, n_fft, hop, win_length, center, length, normalize, shift, out, dev)
    B.check(B.lib().bhw_istft_ola_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), ctypes.byref(s), flags,
                                             ctypes.c_void_p(yr.data_ptr()), ctypes.c_void_p(out.data_ptr())))
    return out


# ---- fused window and real FFT: the spectrum rows in one launch ---------------------------------------------------------------------------

def _fft_check(fft, what="fft"):
    if fft not in ("torch", "fused"):
        raise ValueError(f"{what} must be 'torch' or 'fused', got {fft!r}")
    return fft == "fused"


def _fft_input(torch, x, n_fft, dev):
    """The checks every fused call makes on (x, n_fft): real float32 (T,) or (B, T) on `dev`, n_fft a supported power of two."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a float32 CUDA tensor on the call's device")
    if x.dtype != torch.float32:
        raise ValueError(f"the fused FFT takes real float32 input, got {x.dtype} (complex input: fft='torch' / stft_frames + torch.fft)")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    if not B.fft_supported(n_fft):
        raise ValueError(f"the fused FFT takes n_fft a power of two in {B.FFT_MIN_N}..{B.FFT_MAX_N}, got {int(n_fft)}")


def _cfft_input(torch, x, n_fft, dev):
    """_fft_input for the I/Q calls: complex64 (T,) or (B, T), n_fft a power of two the complex kernel takes.  The device is checked
    at the launch (_cfft_launch), after every check that needs none."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.complex64:
        got = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"the fused complex FFT takes complex64 input, got {got} (real input: stft / spectrogram)")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    if not B.cfft_supported(n_fft):
        raise ValueError(f"the fused complex FFT takes n_fft a power of two in {B.CFFT_MIN_N}..{B.CFFT_MAX_N}, got {int(n_fft)}")


def _cmfft_input(torch, x, n_fft, dev):
    """_cfft_input for the mixed-radix I/Q calls: complex64 (T,) or (B, T), n_fft one the mixed-radix complex kernel takes."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.complex64:
        got = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"the mixed-radix fused complex FFT takes complex64 input, got {got} (real input: stft_mixed / spectrogram_mixed)")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    n = int(n_fft)
    if n > 0 and n & (n - 1) == 0:
        raise ValueError(f"n_fft {n} is a power of two: bhw.stft_iq / bhw.spectrogram_iq transform it (one transform per n_fft)")
    if not B.cmfft_supported(n):
        raise ValueError(f"the mixed-radix fused complex FFT takes n_fft 2^a·3^b·5^c in {B.CMFFT_MIN_N}..{B.CMFFT_MAX_N}, got {n}")


def _fft_out(torch, out, shape, x, dtype=None):
    """The output tensor and its strides in floats: allocated packed, or the caller's `out` of `shape` and `dtype` (complex64 spectrum
    rows by default, float32 for the spectrogram), the last axis contiguous, rows and signals apart; the gaps of a wider buffer are
    left alone."""
    dtype = torch.complex64 if dtype is None else dtype
    floats = 2 if dtype == torch.complex64 else 1
    nb, F, K = shape[-3] if len(shape) == 3 else 1, shape[-2], shape[-1]
    if out is None:
        return torch.empty(shape, dtype=dtype, device=x.device), 0, 0
    ok = isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == x.device and tuple(out.shape) == tuple(shape) \
        and not out.is_conj() and not out.is_neg() and out.stride(-1) == 1
    if ok and F > 1:
        ok = out.stride(-2) >= K
    if ok and len(shape) == 3 and nb > 1:
        ok = out.stride(0) >= (F - 1) * (out.stride(-2) if F > 1 else K) + K
    if not ok:
        name = str(dtype).replace("torch.", "")
        last = "bins" if floats == 2 else "columns"
        raise ValueError(f"out must be a {name} tensor of shape {tuple(shape)} on x's device, contiguous along the {last}, rows and signals apart")
    return out, (out.stride(-2) * floats if F > 1 else 0), (out.stride(0) * floats if len(shape) == 3 and nb > 1 else 0)


def _fft_launch(torch, params, L, s, flags, xr, out, dev, table):
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(xr.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_stft_fft_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(B.lib().bhw_stft_fft_f32_from_table(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev, check=_fft_input):
    """The input checks and the framing every fused forward call shares (stft, spectrogram, stft_iq, spectrogram_iq): (n_fft, L, the
    x read, its (nb, T), frames, and the descriptor's hop, col0, pad, pad_mode).  check: _fft_input, _cfft_input for I/Q input, or the
    mixed-radix ones (_mfft_input, _cmfft_input)."""
    n_fft, L, col0 = _stft_window(params, n_fft, win_length)
    check(torch, x, n_fft, dev)
    hop = int(hop)
    if hop < 1:
        raise ValueError("hop must be >= 1")
    if pad_mode not in _PAD_MODES:
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    if detrend:
        if center:
            raise ValueError("detrend=True forms Welch segments (no padding, the window at column 0): pass center=False")
        pad, col0, mode, reach = 0, 0, 0, L
    else:
        pad, mode = (n_fft // 2 if center else 0), _PAD_MODES[pad_mode]
        reach = n_fft
        if pad and pad_mode == "reflect" and pad >= T:
            raise ValueError(f"reflect padding needs pad {pad} < T = {T} (n_fft // 2 < the signal's length)")
    if nb < 1 or T + 2 * pad < reach:
        raise ValueError(f"zero frames: T + 2 * pad = {T + 2 * pad} < {reach}" if nb else "zero signals")
    frames = 1 + (T + 2 * pad - reach) // hop
    xb = _stft_input(xb, (T,))
    return n_fft, L, xb, nb, T, frames, dict(hop=hop, col0=col0, pad=pad, pad_mode=mode)


def _stft(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, out, dev, table):
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev)
    K = n_fft // 2 + 1
    out, ys, ybs = _fft_out(torch, out, (nb, frames, K) if x.dim() == 2 else (frames, K), x)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                    x_stride=xb.stride(0) if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    return _fft_launch(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend else 0, xb, out, dev, table)


def stft(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, out=None):
    """The short-time Fourier transform of a batch in ONE launch (bhw_stft_fft_f32_device): x (T,) or (B, T), real float32, framed
    and windowed exactly as stft_frames() does (center, pad_mode, the window of win_length centred in an n_fft row) and transformed
    in the same kernel by a float32 FFT in LDS, so neither the windowed frames nor a second pass over x ever reach memory.  Returns
    complex64 (B, F, K) or (F, K) for 1-D x, K = n_fft // 2 + 1, with torch.fft.rfft's sign and no scaling; `.transpose(-1, -2)` of
    it is the layout of torch.stft(x, n_fft, hop, win_length, window=v, center=center, pad_mode=pad_mode, return_complex=True).
    detrend=True (needs center=False) forms scipy's Welch segments instead: no padding, frames = 1 + (T - win_length) // hop, each
    frame's mean removed (the fixed-order binary64 sum of welch_frames), the window at column 0 and zeros up to n_fft.  n_fft: a
    power of two in 16..4096 (ValueError otherwise; complex x too).  The rows the FFT sees are bit for bit those of stft_frames /
    welch_frames; the FFT itself is accurate to a float32 FFT's error, not pinned bit for bit.  `out`: complex64 of the returned
    shape, bins contiguous, rows and signals apart (its gaps are left alone)."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _stft(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, out, x.device.index, None)


# ---- fused window and complex FFT for I/Q input ---------------------------------------------------------------------------------------------

def _stft_iq(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, dev, table, power, mixed=False):
    """stft_iq / spectrogram_iq (power), or with `mixed` stft_iq_mixed / spectrogram_iq_mixed: the same front, the other kernel."""
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev,
                                                 _cmfft_input if mixed else _cfft_input)
    shape = (nb, frames, n_fft) if x.dim() == 2 else (frames, n_fft)
    out, ys, ybs = _fft_out(torch, out, shape, x, torch.float32 if power else torch.complex64)
    if not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a complex64 CUDA tensor on the call's device")
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], channels=2, shift=shift,
                    x_stride=xb.stride(0) * 2 if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    flags = (B.WELCH_DETREND_CONSTANT if detrend else 0) | (B.CFFT_POWER if power else 0) | (B.CFFT_SHIFT if fftshift else 0)
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(xb.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    L_ = B.lib()
    device_call, table_call = (L_.bhw_stft_cmfft_f32_device, L_.bhw_stft_cmfft_f32_from_table) if mixed else \
        (L_.bhw_stft_cfft_f32_device, L_.bhw_stft_cfft_f32_from_table)
    if table is None:
        B.check(device_call(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(table_call(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def stft_iq(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, fftshift=False,
            out=None):
    """The short-time Fourier transform of a batch of complex (I/Q) signals in ONE launch (bhw_stft_cfft_f32_device): x (T,) or
    (B, T), complex64, framed and windowed exactly as stft_frames() does for complex input (center, pad_mode, the window of
    win_length centred in an n_fft row, one coefficient for both parts of a sample) and transformed in the same kernel by a float32
    complex FFT in LDS, so neither the windowed frames nor a second pass over x ever reach memory.  Returns complex64 (B, F, n_fft)
    or (F, n_fft) for 1-D x: all n_fft bins, torch.fft.fft's sign and no scaling; `.transpose(-1, -2)` of it is
    torch.stft(x, n_fft, hop, win_length, window=v, center=center, pad_mode=pad_mode, onesided=False, return_complex=True).
    detrend=True (needs center=False) forms scipy's Welch segments instead: no padding, frames = 1 + (T - win_length) // hop, the
    mean of each part removed (the fixed-order binary64 sums of welch_frames), the window at column 0 and zeros up to n_fft;
    welch_psd(stft_iq(..., detrend=True, center=False), scale, nfft=n_fft, onesided=False) is the fused two-sided Welch estimate.
    fftshift=True writes bin (j + n_fft // 2) % n_fft to column j: torch.fft.fftshift along the bins, the same values.  n_fft: a
    power of two in 16..2048 (ValueError otherwise; a real or complex128 x too: stft() takes real input).  The rows the FFT sees are
    bit for bit those of stft_frames / welch_frames; the FFT itself is accurate to a float32 FFT's error, not pinned bit for bit.
    `out`: complex64 of the returned shape, bins contiguous, rows and signals apart (its gaps are left alone)."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _stft_iq(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, dev, None, False)


def spectrogram_iq(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                   fftshift=False, out=None):
    """The two-sided power spectrogram of a batch of complex (I/Q) signals in ONE launch (bhw_stft_cfft_f32_device with
    BHW_CFFT_POWER): the arguments, rows and transform of stft_iq(), and each bin written as fl32(re^2 + im^2), taken in binary64, of
    the float32 pair stft_iq() would have written -- bit for bit -- so the complex spectrum never reaches memory.  Returns float32
    (B, F, n_fft) or (F, n_fft) for 1-D x; `.transpose(-1, -2)` gives the (..., freq, time) layout; fftshift=True puts the zero
    frequency at column n_fft // 2.  A filter bank on these rows is not built.  `out`: float32 of the returned shape, columns
    contiguous, rows and signals apart (its gaps are left alone)."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _stft_iq(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, dev, None, True)


def stft_iq_mixed(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, fftshift=False,
                  out=None):
    """stft_iq() for the row lengths complex baseband uses and a power-of-two transform refuses, in ONE launch
    (bhw_stft_cmfft_f32_device): n_fft 2^a·3^b·5^c in 16..2047 and not a power of two, odd lengths included -- 1536, 1200, 600, 300,
    180, 1000, 2000, 480, 960, 75.  The arguments, the shapes, the `out` rules and the errors are stft_iq()'s: x (T,) or (B, T),
    complex64, framed and windowed exactly as stft_frames() / welch_frames() do for complex input (their rows bit for bit) and
    transformed in the same kernel by a float32 mixed-radix complex FFT in LDS (radix-5, -3, -4 and -2 Stockham passes over n_fft
    points).  Returns complex64 (B, F, n_fft) or (F, n_fft); `stft_iq_mixed(p, x, n, hop).transpose(-1, -2)` is
    torch.stft(x, n, hop, window=v, onesided=False, return_complex=True).  detrend=True (needs center=False) forms scipy's Welch
    segments, and welch_psd(stft_iq_mixed(..., detrend=True, center=False), scale, nfft=n_fft, onesided=False) is the two-sided Welch
    estimate at such an nfft.  fftshift=True writes bin k to column (k + n_fft // 2) % n_fft: torch.fft.fftshift along the bins, for
    an odd n_fft too.  A power-of-two n_fft raises ValueError (bhw.stft_iq transforms it: one transform per n_fft); any other
    unsupported n_fft and a real or complex128 x raise ValueError too.  The FFT is accurate to a float32 FFT's error, not pinned bit
    for bit."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _stft_iq(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, dev, None, False, True)


def spectrogram_iq_mixed(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                         fftshift=False, out=None):
    """spectrogram_iq() at the n_fft of stft_iq_mixed() (bhw_stft_cmfft_f32_device with BHW_CFFT_POWER): each bin fl32(re^2 + im^2),
    taken in binary64, of the float32 pair stft_iq_mixed() would have written -- bit for bit.  Returns float32 (B, F, n_fft) or
    (F, n_fft); fftshift=True puts the zero frequency at column n_fft // 2.  The arguments, `out` rules and errors are
    spectrogram_iq()'s; a power-of-two n_fft raises ValueError (bhw.spectrogram_iq transforms it)."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _stft_iq(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, dev, None, True, True)


def _ifft_input(torch, Y, dev):
    """The input check of istft(): one-sided complex64 spectra (frames, K) or (B, frames, K) on the call's device."""
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda or Y.device.index != dev:
        raise ValueError("Y must be a complex64 CUDA tensor on the call's device")
    if Y.dtype != torch.complex64:
        raise ValueError(f"the fused inverse FFT takes one-sided complex64 spectra, got {Y.dtype}")
    if Y.dim() not in (2, 3):
        raise ValueError("Y must be (frames, K) or (B, frames, K)")


def _icfft_input(torch, Y, dev):
    """_ifft_input for istft_iq(): two-sided complex64 spectra (frames, n_fft) or (B, frames, n_fft).  The device is checked at the
    launch (_istft), after every check that needs none."""
    if not isinstance(Y, torch.Tensor) or Y.dtype != torch.complex64:
        got = Y.dtype if isinstance(Y, torch.Tensor) else type(Y).__name__
        raise ValueError(f"the fused inverse complex FFT takes two-sided complex64 spectra, got {got} (one-sided spectra: istft)")
    if Y.dim() not in (2, 3):
        raise ValueError("Y must be (frames, n_fft) or (B, frames, n_fft)")


def _imfft_input(torch, Y, dev):
    """_ifft_input for istft_mixed(): one-sided complex64 spectra (frames, K) or (B, frames, K).  The device is checked at the launch
    (_istft), after every check that needs none."""
    if not isinstance(Y, torch.Tensor) or Y.dtype != torch.complex64:
        got = Y.dtype if isinstance(Y, torch.Tensor) else type(Y).__name__
        raise ValueError(f"the mixed-radix fused inverse FFT takes one-sided complex64 spectra, got {got}")
    if Y.dim() not in (2, 3):
        raise ValueError("Y must be (frames, K) or (B, frames, K)")


def _icmfft_input(torch, Y, dev):
    """_icfft_input for istft_iq_mixed(): two-sided complex64 spectra (frames, n_fft) or (B, frames, n_fft).  The device is checked at
    the launch (_istft), after every check that needs none."""
    if not isinstance(Y, torch.Tensor) or Y.dtype != torch.complex64:
        got = Y.dtype if isinstance(Y, torch.Tensor) else type(Y).__name__
        raise ValueError(f"the mixed-radix fused inverse complex FFT takes two-sided complex64 spectra, got {got} (one-sided spectra: "
                         f"istft_mixed)")
    if Y.dim() not in (2, 3):
        raise ValueError("Y must be (frames, n_fft) or (B, frames, n_fft)")


def _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, dev, table, check=_ifft_input,
           dtype=None, fftshift=False):
    """The body istft(), istft_mixed(), istft_iq() and istft_iq_mixed() share.  check: _ifft_input, _imfft_input for the mixed-radix
    lengths, _icfft_input for I/Q output or _icmfft_input for I/Q output at the mixed-radix lengths; dtype: the output's, float32 (the
    one-sided spectra of istft) by default, complex64 for the two-sided spectra of istft_iq and istft_iq_mixed."""
    dtype = torch.float32 if dtype is None else dtype
    iq = dtype == torch.complex64
    mixed = check is _imfft_input
    cmixed = check is _icmfft_input
    check(torch, Y, dev)
    n_fft, L, col0 = _stft_window(params, n_fft, win_length)
    if cmixed and B.cfft_supported(n_fft):
        raise ValueError(f"n_fft {n_fft} is a power of two: bhw.istft_iq transforms it (one transform per n_fft)")
    if cmixed and not B.cmfft_supported(n_fft):
        raise ValueError(f"the mixed-radix fused inverse complex FFT takes n_fft = 2^a 3^b 5^c in {B.CMFFT_MIN_N}..{B.CMFFT_MAX_N} that is "
                         f"no power of two, got {n_fft}")
    if iq and not cmixed and not B.cfft_supported(n_fft):
        raise ValueError(f"the fused inverse complex FFT takes n_fft a power of two in {B.CFFT_MIN_N}..{B.CFFT_MAX_N}, got {n_fft}")
    if mixed and B.fft_supported(n_fft):
        raise ValueError(f"n_fft {n_fft} is a power of two: bhw.istft transforms it (one transform per n_fft)")
    if mixed and not B.mfft_supported(n_fft):
        raise ValueError(f"the mixed-radix fused inverse FFT takes an even n_fft = 2^a 3^b 5^c in {B.MFFT_MIN_N}..{B.MFFT_MAX_N} that is "
                         f"no power of two, got {n_fft}")
    if not iq and not mixed and not B.fft_supported(n_fft):
        raise ValueError(f"the fused inverse FFT takes n_fft a power of two in {B.FFT_MIN_N}..{B.FFT_MAX_N}, got {n_fft}")
    hop = int(hop)
    if hop < 1:
        raise ValueError("hop must be >= 1")
    if not center and L < n_fft:
        raise ValueError("center=False with win_length < n_fft: the first outputs have no window under them")
    Yb = Y if Y.dim() == 3 else Y.unsqueeze(0)
    nb, frames, K = Yb.shape
    if iq and K != n_fft:
        raise ValueError(f"Y rows hold {K} bins, the two-sided spectrum of n_fft {n_fft} has {n_fft} (one-sided spectra: "
                         f"{'istft_mixed' if cmixed else 'istft'})")
    if not iq and K != n_fft // 2 + 1:
        raise ValueError(f"Y rows hold {K} bins, n_fft // 2 + 1 is {n_fft // 2 + 1}")
    if frames < 1 or nb < 1:
        raise ValueError("zero frames")
    pad = n_fft // 2 if center else 0
    length = n_fft + hop * (frames - 1) - 2 * pad if length is None else int(length)
    if length < 0:
        raise ValueError(f"length {length} < 0")
    Yb = _stft_input(Yb, ((frames - 1) * max(Yb.stride(1), K) + K, K))
    shape = (nb, length) if Y.dim() == 3 else (length,)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=Y.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != Y.device or not out.is_contiguous() \
            or out.is_neg() or out.is_conj() or tuple(out.shape) != shape:
        raise ValueError(f"out must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {shape} on Y's device")
    if (iq or mixed) and (not Y.is_cuda or Y.device.index != dev):
        raise ValueError("Y must be a complex64 CUDA tensor on the call's device")
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, length, frames, hop, n_fft, col0=col0, pad=pad, shift=shift, channels=2 if iq else 1,
                    y_stride=Yb.stride(1) * 2 if frames > 1 else 0, y_batch_stride=Yb.stride(0) * 2 if nb > 1 else 0)
    flags = (B.OLA_NORMALIZE if normalize else 0) | (B.CFFT_SHIFT if fftshift else 0)
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(Yb.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    L_ = B.lib()
    device_call, table_call = (L_.bhw_istft_cmfft_f32_device, L_.bhw_istft_cmfft_f32_from_table) if cmixed else \
        (L_.bhw_istft_cfft_f32_device, L_.bhw_istft_cfft_f32_from_table) if iq else \
        (L_.bhw_istft_mfft_f32_device, L_.bhw_istft_mfft_f32_from_table) if mixed else \
        (L_.bhw_istft_fft_f32_device, L_.bhw_istft_fft_f32_from_table)
    if table is None:
        B.check(device_call(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(table_call(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def istft(params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, out=None):
    """The inverse short-time Fourier transform of a batch in ONE launch (bhw_istft_fft_f32_device): Y (B, F, K) or (F, K), complex64,
    K = n_fft // 2 + 1 -- the layout stft() returns.  Every row is transformed as torch.fft.irfft(Y, n=n_fft) does (same sign and
    1 / n_fft scaling; the imaginary parts of bins 0 and n_fft / 2 are ignored) by a float32 FFT in LDS, and summed exactly as
    istft_overlap_add() sums time rows: in ascending frame order in binary64, times v (window(params, win_length,
    dtype=torch.float32, shift=shift)), and with normalize=True divided by the window envelope (+0.0 where no frame reaches).  The time
    rows never reach memory.  length defaults to torch.istft's n_fft + hop * (frames - 1) - 2 * pad; outputs past the frames' extent are
    +0.0.  Returns float32 (B, length), or (length,) for 2-D Y.  istft(params, S.transpose(-1, -2), ...) is torch.istft(S, n_fft, hop,
    win_length, window=v, center=center, length=length) to a float32 FFT's error.  n_fft: a power of two in 16..4096 (ValueError
    otherwise; a real or complex128 Y too).  Y is read in place when its bins are contiguous and its rows and signals apart; a
    transposed view (of a torch.stft result, say), a broadcast or a lazy conjugate is copied first.  `out`: a contiguous float32 tensor
    of the returned shape.  With heavy overlap and little work (see describe_istft_fft) few workgroups run; torch.fft.irfft +
    istft_overlap_add remains for that case, and this call does not reroute to it."""
    torch = _torch()
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda:
        raise ValueError("Y must be a complex64 CUDA tensor")
    return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, Y.device.index, None)


def istft_mixed(params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, out=None):
    """istft() at the n_fft of stft_mixed() in ONE launch (bhw_istft_mfft_f32_device): Y (B, F, K) or (F, K), complex64,
    K = n_fft // 2 + 1 -- the layout stft_mixed() returns -- for n_fft even, 2^a·3^b·5^c, in 16..4095 and not a power of two (400, 480,
    960, 1000, 1200, 1920, ...; ValueError otherwise, and a power of two names istft()).  Every row is transformed as
    torch.fft.irfft(Y, n=n_fft) does by a float32 mixed-radix FFT in LDS (the 1 / n_fft scaling is one float32 multiply by
    fl32(1 / n_fft); the imaginary parts of bins 0 and n_fft / 2 are ignored) and summed exactly as istft_overlap_add() sums time rows:
    in ascending frame order in binary64, times v (window(params, win_length, dtype=torch.float32, shift=shift)), and with
    normalize=True divided by the window envelope (+0.0 where no frame reaches).  The time rows never reach memory.  Keywords, the
    default length, the treatment of views and `out` are istft()'s.  istft_mixed(params, S.transpose(-1, -2), 400, 160) is
    torch.istft(S, 400, 160, window=v) to a float32 FFT's error.  With heavy overlap and little work (see describe_istft_mfft) few
    workgroups run; torch.fft.irfft + istft_overlap_add remains for that case, and this call does not reroute to it."""
    torch = _torch()
    dev = Y.device.index if isinstance(Y, torch.Tensor) and Y.is_cuda else None
    return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, dev, None, _imfft_input)


def istft_iq(params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, fftshift=False, out=None):
    """The inverse short-time Fourier transform of a batch of complex (I/Q) signals in ONE launch (bhw_istft_cfft_f32_device): Y
    (B, F, n_fft) or (F, n_fft), complex64, all n_fft bins -- the layout stft_iq() returns.  Every row is transformed as
    torch.fft.ifft does (same sign and 1 / n_fft scaling) by a float32 complex FFT in LDS, and summed exactly as istft_overlap_add()
    sums complex time rows: in ascending frame order in binary64 per part, times v (window(params, win_length, dtype=torch.float32,
    shift=shift)), and with normalize=True divided by the window envelope (+0.0 where no frame reaches).  The time rows never reach
    memory.  fftshift=True reads rows whose column j holds bin (j + n_fft // 2) % n_fft, what stft_iq(fftshift=True) writes.  length
    defaults to torch.istft's n_fft + hop * (frames - 1) - 2 * pad; outputs past the frames' extent are +0.0.  Returns complex64
    (B, length), or (length,) for 2-D Y.  istft_iq(params, S.transpose(-1, -2), ...) is torch.istft(S, n_fft, hop, win_length,
    window=v, center=center, length=length, onesided=False, return_complex=True) to a float32 FFT's error.  n_fft: a power of two in
    16..2048 (ValueError otherwise; a real, complex128 or one-sided Y too: istft() takes one-sided spectra).  Y is read in place when
    its bins are contiguous and its rows and signals apart; a transposed view, a broadcast or a lazy conjugate is copied first.
    `out`: a contiguous complex64 tensor of the returned shape.  With heavy overlap and little work (see describe_istft_cfft) few
    workgroups run; torch.fft.ifft + istft_overlap_add remains for that case, and this call does not reroute to it."""
    torch = _torch()
    dev = Y.device.index if isinstance(Y, torch.Tensor) and Y.is_cuda else None
    return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, dev, None, _icfft_input,
                  torch.complex64, fftshift)


def istft_iq_mixed(params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, fftshift=False,
                   out=None):
    """istft_iq() at the n_fft of stft_iq_mixed() in ONE launch (bhw_istft_cmfft_f32_device): Y (B, F, n_fft) or (F, n_fft), complex64,
    all n_fft bins -- the layout stft_iq_mixed() returns -- for n_fft 2^a·3^b·5^c in 16..2047 and not a power of two, odd lengths
    included (1536, 1200, 600, 300, 1000, 2000, 480, 960, 75, ...; ValueError otherwise, and a power of two names istft_iq()).  Every
    row is transformed as torch.fft.ifft does by a float32 mixed-radix complex FFT in LDS (the 1 / n_fft scaling is one float32
    multiply of each part by fl32(1 / n_fft)) and summed exactly as istft_overlap_add() sums complex time rows: in ascending frame
    order in binary64 per part, times v (window(params, win_length, dtype=torch.float32, shift=shift)), and with normalize=True divided
    by the window envelope (+0.0 where no frame reaches).  The time rows never reach memory.  fftshift=True reads rows whose column
    (k + n_fft // 2) % n_fft holds bin k, what stft_iq_mixed(fftshift=True) writes (torch.fft.fftshift along the bins, for an odd
    n_fft too).  Keywords, the default length, the treatment of views and `out` are istft_iq()'s.  With heavy overlap and little work
    (see describe_istft_cmfft) few workgroups run; torch.fft.ifft + istft_overlap_add remains for that case, and this call does not
    reroute to it."""
    torch = _torch()
    dev = Y.device.index if isinstance(Y, torch.Tensor) and Y.is_cuda else None
    return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, dev, None, _icmfft_input,
                  torch.complex64, fftshift)


# ---- fused power and filter-bank spectrogram ---------------------------------------------------------------------------------------------

# ---- fused STFT, spectral mask and inverse STFT: analysis, modify and synthesis in one launch ----------------------------------------------

def _mask_fft_refusals(torch, x, mask, n_fft):
    """What stft_mask_istft() does not take, refused naming the calls that do, before any check that needs a device."""
    if isinstance(mask, torch.Tensor) and mask.is_complex():
        raise ValueError("the fused mask takes real float32 gains; complex gains are not built: bhw.stft, a complex multiply and bhw.istft "
                         "apply them")
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"the fused mask takes real float32 input, got {x.dtype} (I/Q input: bhw.stft_iq, a multiply and bhw.istft_iq)")
    n = int(n_fft)
    if n > 0 and n & (n - 1) and B.mfft_supported(n):
        raise ValueError(f"the fused mask takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (a mixed-radix n_fft: "
                         f"bhw.stft_mixed, a multiply and bhw.istft_mixed)")
    if B.fft_supported(n) and not B.mask_fft_supported(n):
        raise ValueError(f"the fused mask takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (bhw.stft, a multiply and "
                         f"bhw.istft take it)")


def _mask_gains(torch, mask, nb, frames, K, dev, complex_gains=False, iq=False):
    """The gains as the kernel reads them: (the tensor read, g_stride, g_batch_stride).  mask: real float32 -- complex64 with
    complex_gains, the strides then counting (re, im) pairs, as torch counts them -- (K,), (F, K) or (1 | B, 1 | F, K), its last axis
    contiguous.  An axis of size 1 or of stride 0 (an expand() view) becomes a zero stride and is never materialised; rows or signals
    that overlap in memory some other way are copied first.  A lazy conjugate is resolved first.  iq: the I/Q calls, whose rows hold
    K = n_fft gains and say so."""
    want = torch.complex64 if complex_gains else torch.float32
    if not isinstance(mask, torch.Tensor) or mask.dtype != want or not mask.is_cuda or mask.device.index != dev:
        raise ValueError("mask must be a complex64 CUDA tensor on the call's device" if complex_gains else
                         "mask must be a real float32 CUDA tensor on the call's device")
    if iq and (mask.dim() not in (1, 2, 3) or mask.shape[-1] != K):
        raise ValueError(f"mask must be (K,), (F, K) or (1 | B, 1 | F, K) with K = n_fft = {K} (I/Q input: every bin takes a gain), got "
                         f"{tuple(mask.shape)}")
    if mask.dim() not in (1, 2, 3) or mask.shape[-1] != K:
        raise ValueError(f"mask must be (K,), (F, K) or (1 | B, 1 | F, K) with K = n_fft // 2 + 1 = {K}, got {tuple(mask.shape)}")
    m = mask.resolve_conj().resolve_neg()
    while m.dim() < 3:
        m = m.unsqueeze(0)
    if m.shape[0] not in (1, nb) or m.shape[1] not in (1, frames):
        raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to (B, F, K) = {(nb, frames, K)}")
    if K > 1 and m.stride(2) != 1:
        raise ValueError("mask must be contiguous along its last axis (the bins)")
    gs = m.stride(1) if m.shape[1] > 1 else 0
    gbs = m.stride(0) if m.shape[0] > 1 else 0
    if (gs and gs < K) or (gbs and gbs < (frames - 1) * gs + K):
        m = m.contiguous()
        gs = m.stride(1) if m.shape[1] > 1 else 0
        gbs = m.stride(0) if m.shape[0] > 1 else 0
    return m, gs, gbs


def stft_mask_istft(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                    shift=None, out=None, table=None):
    """A time-frequency mask applied to a batch in ONE launch (bhw_mask_fft_f32_device): stft(), a real gain per bin and istft() with
    neither spectrum in memory.  x (T,) or (B, T), float32; mask real float32, broadcastable to (B, F, K) by torch's rules -- (K,),
    (F, K) or (1 | B, 1 | F, K), K = n_fft // 2 + 1, F the frames stft() gives, the last axis contiguous.  A broadcast axis, an
    expand() view included, is never materialised.  Returns float32 (B, length), or (length,) for 1-D x; length defaults to T.  The
    result equals

        bhw.istft(params, bhw.stft(params, x, n_fft, hop, ...) * mask[..., None], n_fft, hop, ..., length=length, normalize=normalize)

    BIT FOR BIT: the rows are stft()'s words, each part times its gain is rounded once, and the sum is istft()'s.  n_fft: a power of
    two in 16..2048.  ValueError naming the calls that take it: a complex mask (stft + a complex multiply + istft), a mixed-radix n_fft
    (stft_mixed + istft_mixed), complex x (stft_iq + istft_iq), 4096 (stft + istft).  `out`: a contiguous float32 tensor of the
    returned shape; it may not share memory with x or mask.  `table`: a ResidentTable of these params to gather the window
    coefficients from (bhw_mask_fft_f32_from_table: no allocation by the library, no synchronisation, capturable on its first call),
    or None (the library form: capturable with no warm call).  stft_mask_istft_mixed() is this call at a mixed-radix n_fft,
    stft_cmask_istft() this call with a complex gain per bin, and stft_mask_istft_iq() this call for complex (I/Q) x in one launch."""
    torch = _torch()
    _mask_fft_refusals(torch, x, mask, n_fft)
    return _stft_mask_istft(torch, params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                            _fft_input, "bhw_mask_fft_f32_device", "bhw_mask_fft_f32_from_table")


def _stft_mask_istft(torch, params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table, check, device_call,
                     table_call, complex_gains=False, iq=False, fftshift=False):
    """What stft_mask_istft(), stft_mask_istft_mixed(), their complex-gain siblings and the four I/Q calls share after their refusals:
    the input checks (check: _fft_input or _mfft_input; _cfft_input or _cmfft_input with iq), the two descriptors, the gains
    (complex_gains: complex64, strides in pairs; iq: K = n_fft of them a row, fftshift: their columns on a centred axis) and the one
    call."""
    if table is not None:
        if not isinstance(table, ResidentTable):
            raise ValueError("table must be a ResidentTable or None")
        dev, handle = table.device, table._live()
    else:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("x must be a complex64 CUDA tensor" if iq else "x must be a float32 CUDA tensor")
        dev, handle = x.device.index, None
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, False, dev, check)
    if not center and L < n_fft:
        raise ValueError("center=False with win_length < n_fft: the first outputs have no window under them")
    if iq and (not x.is_cuda or x.device.index != dev):
        raise ValueError("x must be a complex64 CUDA tensor on the call's device")
    K = n_fft if iq else n_fft // 2 + 1
    C = 2 if iq else 1
    g, gs, gbs = _mask_gains(torch, mask, nb, frames, K, dev, complex_gains, iq)
    length = T if length is None else int(length)
    if length < 0:
        raise ValueError(f"length {length} < 0")
    out = _stft_out(torch, out, (nb, length) if x.dim() == 2 else (length,), x, "x")
    shift = params.dat_width - 1 if shift is None else int(shift)
    sa = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift, channels=C,
                     x_stride=xb.stride(0) * C if nb > 1 else 0)
    ss = B.make_stft(nb, length, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], shift=shift, channels=C)
    flags = (B.OLA_NORMALIZE if normalize else 0) | (B.CFFT_SHIFT if fftshift else 0)
    tail = (ctypes.byref(sa), ctypes.byref(ss), flags, ctypes.c_void_p(xb.data_ptr()),
            ctypes.c_void_p(g.data_ptr()), gs, gbs, ctypes.c_void_p(out.data_ptr()))
    if handle is None:
        B.check(getattr(B.lib(), device_call)(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(getattr(B.lib(), table_call)(handle, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def _mask_mfft_refusals(torch, x, mask, n_fft):
    """What stft_mask_istft_mixed() does not take, refused naming the calls that do, before any check that needs a device."""
    if isinstance(mask, torch.Tensor) and mask.is_complex():
        raise ValueError("the mixed-radix fused mask takes real float32 gains; complex gains are not built: bhw.stft_mixed, a complex "
                         "multiply and bhw.istft_mixed apply them")
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"the mixed-radix fused mask takes real float32 input, got {x.dtype} (I/Q input: bhw.stft_iq_mixed, a multiply "
                         f"and bhw.istft_iq_mixed)")
    n = int(n_fft)
    if B.mask_fft_supported(n):
        raise ValueError(f"n_fft {n} is a power of two: bhw.stft_mask_istft takes it (one transform per n_fft)")
    if B.fft_supported(n):
        raise ValueError(f"n_fft {n} is a power of two above {B.MASK_FFT_MAX_N}: bhw.stft, a multiply and bhw.istft take it")
    if n > B.MASK_MFFT_MAX_N and B.mfft_supported(n):
        raise ValueError(f"the mixed-radix fused mask takes n_fft even 2^a·3^b·5^c in {B.MFFT_MIN_N}..{B.MASK_MFFT_MAX_N}, got {n} "
                         f"(bhw.stft_mixed, a multiply and bhw.istft_mixed take it)")


def stft_mask_istft_mixed(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                          shift=None, out=None, table=None):
    """stft_mask_istft() at the n_fft of stft_mixed() in ONE launch (bhw_mask_mfft_f32_device): n_fft even, 2^a·3^b·5^c, no power of two,
    from 18 to 2000 -- 320, 400, 480, 960, 1000, 1200, 1920.  The arguments, the shapes, the `out` rules and the mask layouts are
    stft_mask_istft()'s: x (T,) or (B, T), float32; mask real float32 (K,), (F, K) or (1 | B, 1 | F, K), K = n_fft // 2 + 1, a
    broadcast axis (an expand() view included) never materialised.  The result equals

        bhw.istft_mixed(params, bhw.stft_mixed(params, x, n_fft, hop, ...) * mask[..., None], n_fft, hop, ..., length=length,
                        normalize=normalize)

    BIT FOR BIT.  ValueError naming the calls that take it: a power of two (stft_mask_istft), an n_fft of 2048 or more (stft_mixed, a
    multiply and istft_mixed), complex x (stft_iq_mixed + istft_iq_mixed), a complex mask (stft_mixed + a complex multiply +
    istft_mixed).  `table`: a ResidentTable of these params (bhw_mask_mfft_f32_from_table: no allocation by the library, no
    synchronisation, capturable on its first call), or None (the library form: capturable with no warm call).
    stft_cmask_istft_mixed() is this call with a complex gain per bin, stft_mask_istft_iq_mixed() this call for complex (I/Q) x."""
    import torch as host_torch                            # the refusals look at no device: they come before _torch() asks for one
    _mask_mfft_refusals(host_torch, x, mask, n_fft)
    torch = _torch()
    return _stft_mask_istft(torch, params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                            _mfft_input, "bhw_mask_mfft_f32_device", "bhw_mask_mfft_f32_from_table")


# ---- the same with a complex gain per bin ------------------------------------------------------------------------------------------------

def _cmask_refusals(torch, x, mask, n_fft, mixed):
    """What stft_cmask_istft() (mixed False) and stft_cmask_istft_mixed() (mixed True) do not take, refused naming the calls that do,
    before any check that needs a device."""
    what = "the mixed-radix fused complex-gain mask" if mixed else "the fused complex-gain mask"
    tail = "_mixed" if mixed else ""
    if isinstance(mask, torch.Tensor) and not mask.is_complex():
        raise ValueError(f"{what} takes complex64 gains, got {mask.dtype}: bhw.stft_mask_istft{tail} takes real gains")
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"{what} takes real float32 input, got {x.dtype} (I/Q input: bhw.stft_iq{tail}, a complex multiply and "
                         f"bhw.istft_iq{tail})")
    n = int(n_fft)
    if mixed:
        if B.mask_fft_supported(n):
            raise ValueError(f"n_fft {n} is a power of two: bhw.stft_cmask_istft takes it (one transform per n_fft)")
        if B.fft_supported(n):
            raise ValueError(f"n_fft {n} is a power of two above {B.MASK_FFT_MAX_N}: bhw.stft, a complex multiply and bhw.istft take it")
        if n > B.MASK_MFFT_MAX_N and B.mfft_supported(n):
            raise ValueError(f"{what} takes n_fft even 2^a·3^b·5^c in {B.MFFT_MIN_N}..{B.MASK_MFFT_MAX_N}, got {n} (bhw.stft_mixed, a "
                             f"complex multiply and bhw.istft_mixed take it)")
    else:
        if B.mask_mfft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (a mixed-radix n_fft: "
                             f"bhw.stft_cmask_istft_mixed takes it)")
        if n > 0 and n & (n - 1) and B.mfft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (bhw.stft_mixed, a complex "
                             f"multiply and bhw.istft_mixed take it)")
        if B.fft_supported(n) and not B.mask_fft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (bhw.stft, a complex multiply "
                             f"and bhw.istft take it)")


def stft_cmask_istft(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                     shift=None, out=None, table=None):
    """stft_mask_istft() with a COMPLEX gain per bin in ONE launch (bhw_cmask_fft_f32_device): a complex ratio mask, a frequency
    response H[k] as one (K,) row, a fractional delay exp(-2πi·k·d/n_fft), a beamforming weight per bin.  x (T,) or (B, T), float32;
    mask complex64 with the layouts of stft_mask_istft(): (K,), (F, K) or (1 | B, 1 | F, K), K = n_fft // 2 + 1, the last axis
    contiguous; an axis of size 1 or stride 0 (an expand() view) is never materialised, a conjugate view is resolved first.  With
    Y = bhw.stft(params, x, n_fft, hop, ...) and G = mask, the masked spectrum is, in separate float32 operations,

        Z.real = Y.real * G.real - Y.imag * G.imag        Z.imag = Y.real * G.imag + Y.imag * G.real

    -- each of the four products rounded on its own -- and the result equals bhw.istft(params, Z, n_fft, hop, ..., length=length,
    normalize=normalize) BIT FOR BIT.  That is what eager float32 torch operations on the two planes give; it is not promised to
    equal Y * G of torch complex tensors bit for bit (a library's complex multiply may round differently), only to within that
    multiply's rounding.  The imaginary parts of the gains at bins 0 and n_fft / 2 multiply stored zeros and are otherwise unused.
    n_fft: a power of two in 16..2048.  ValueError naming the calls that take it: a real mask (stft_mask_istft), a mixed-radix n_fft
    (stft_cmask_istft_mixed), complex x (stft_iq + istft_iq), 4096 (stft, a complex multiply and istft).  `out`, `table` and the
    other keywords are stft_mask_istft()'s (bhw_cmask_fft_f32_from_table).  stft_cmask_istft_iq() is this call for complex (I/Q) x in
    one launch."""
    import torch as host_torch                            # the refusals look at no device: they come before _torch() asks for one
    _cmask_refusals(host_torch, x, mask, n_fft, False)
    torch = _torch()
    return _stft_mask_istft(torch, params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                            _fft_input, "bhw_cmask_fft_f32_device", "bhw_cmask_fft_f32_from_table", True)


def stft_cmask_istft_mixed(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                           shift=None, out=None, table=None):
    """stft_cmask_istft() at the n_fft of stft_mixed() in ONE launch (bhw_cmask_mfft_f32_device): n_fft even, 2^a·3^b·5^c, no power of
    two, from 18 to 2000 -- 320, 400, 480, 960, 1000, 1200, 1920.  The arguments, the complex64 mask layouts, the four-product formula
    and the statement about torch's complex multiply are stft_cmask_istft()'s, with stft_mixed() and istft_mixed() as the two
    transforms: the result equals istft_mixed() of the masked stft_mixed() rows BIT FOR BIT.  ValueError naming the calls that take
    it: a real mask (stft_mask_istft_mixed), a power of two (stft_cmask_istft), an n_fft of 2048 or more (stft_mixed, a complex
    multiply and istft_mixed), complex x (stft_iq_mixed + istft_iq_mixed).  `table`: bhw_cmask_mfft_f32_from_table.
    stft_cmask_istft_iq_mixed() is this call for complex (I/Q) x in one launch."""
    import torch as host_torch
    _cmask_refusals(host_torch, x, mask, n_fft, True)
    torch = _torch()
    return _stft_mask_istft(torch, params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                            _mfft_input, "bhw_cmask_mfft_f32_device", "bhw_cmask_mfft_f32_from_table", True)


# ---- multichannel filter-and-sum: an STFT per channel, a complex weight per channel and bin, one inverse STFT ------------------------------

def _beam_refusals(torch, x, weights, n_fft, mixed):
    """What stft_beamform_istft() (mixed False) and stft_beamform_istft_mixed() (mixed True) do not take, refused naming what does,
    before any check that needs a device."""
    what = "the mixed-radix fused beamformer" if mixed else "the fused beamformer"
    tail = "_mixed" if mixed else ""
    if isinstance(weights, torch.Tensor) and not weights.is_complex():
        raise ValueError(f"{what} takes complex64 weights, got {weights.dtype}: real gains per channel are not built (weights.to(torch.complex64) "
                         f"applies them; bhw.stft_mask_istft{tail} takes real gains on one channel)")
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"{what} takes real float32 input, got {x.dtype}: the I/Q beamformer is not built (bhw.stft_cmask_istft_iq{tail} per "
                         f"channel and a sum over the channels take it)")
    n = int(n_fft)
    if mixed:
        if B.mask_fft_supported(n):
            raise ValueError(f"n_fft {n} is a power of two: bhw.stft_beamform_istft takes it (one transform per n_fft)")
        if B.fft_supported(n):
            raise ValueError(f"n_fft {n} is a power of two above {B.MASK_FFT_MAX_N}: bhw.stft, the weights and a sum over the channels, and "
                             f"bhw.istft take it")
        if n > B.MASK_MFFT_MAX_N and B.mfft_supported(n):
            raise ValueError(f"{what} takes n_fft even 2^a·3^b·5^c in {B.MFFT_MIN_N}..{B.MASK_MFFT_MAX_N}, got {n} (bhw.stft_mixed, the "
                             f"weights and a sum over the channels, and bhw.istft_mixed take it)")
    else:
        if B.mask_mfft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (a mixed-radix n_fft: "
                             f"bhw.stft_beamform_istft_mixed takes it)")
        if n > 0 and n & (n - 1) and B.mfft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (bhw.stft_mixed, the weights "
                             f"and a sum over the channels, and bhw.istft_mixed take it)")
        if B.fft_supported(n) and not B.mask_fft_supported(n):
            raise ValueError(f"{what} takes n_fft a power of two in {B.FFT_MIN_N}..{B.MASK_FFT_MAX_N}, got {n} (bhw.stft, the weights and a "
                             f"sum over the channels, and bhw.istft take it)")
    if isinstance(x, torch.Tensor) and x.dim() not in (2, 3):
        raise ValueError(f"x must be (C, T) or (B, C, T), got {tuple(x.shape)}")
    if isinstance(x, torch.Tensor) and not 1 <= x.shape[-2] <= B.BEAM_MAX_CH:
        raise ValueError(f"x has {x.shape[-2]} channels: the fused beamformer takes 1..{B.BEAM_MAX_CH}")
    if isinstance(x, torch.Tensor) and isinstance(weights, torch.Tensor):
        C = x.shape[-2]
        if weights.dim() not in (2, 3, 4):
            raise ValueError(f"weights must be (C, K), (C, F, K) or (1 | B, C, 1 | F, K), got {tuple(weights.shape)}")
        ch = weights.dim() - (2 if weights.dim() == 2 else 3)
        if C > 1 and (weights.shape[ch] == 1 or (weights.shape[ch] == C and weights.stride(ch) == 0)):
            raise ValueError("weights are broadcast along the channels: the same weights on every channel are x.sum over the channels "
                             f"and bhw.stft_cmask_istft{tail}; the fused beamformer takes a row per channel")
        if weights.shape[ch] != C:
            raise ValueError(f"weights {tuple(weights.shape)} have {weights.shape[ch]} channels, x has {C}")


def _beam_gains(torch, weights, nb, C, frames, K, dev):
    """The weights as the kernel reads them: (the tensor read, g_stride, g_ch_stride, g_batch_stride), the strides in (re, im) pairs
    as torch counts them.  weights: complex64 (C, K), (C, F, K) or (1 | B, C, 1 | F, K), the last axis contiguous.  A batch or frame
    axis of size 1 or of stride 0 (an expand() view) becomes a zero stride and is never materialised; rows that overlap in memory some
    other way are copied first.  A lazy conjugate is resolved first."""
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.complex64 or not weights.is_cuda or weights.device.index != dev:
        raise ValueError("weights must be a complex64 CUDA tensor on the call's device")
    m = weights.resolve_conj().resolve_neg()
    if m.dim() == 2:
        m = m.unsqueeze(1)
    if m.dim() == 3:
        m = m.unsqueeze(0)
    if m.shape[0] not in (1, nb) or m.shape[1] != C or m.shape[2] not in (1, frames) or m.shape[3] != K:
        raise ValueError(f"weights {tuple(weights.shape)} do not broadcast to (B, C, F, K) = {(nb, C, frames, K)} (K = n_fft // 2 + 1)")
    if K > 1 and m.stride(3) != 1:
        raise ValueError("weights must be contiguous along their last axis (the bins)")

    def strides(t):
        return t.stride(2) if t.shape[2] > 1 else 0, t.stride(1) if C > 1 else 0, t.stride(0) if t.shape[0] > 1 else 0
    gs, gcs, gbs = strides(m)
    rows = (frames - 1) * gs + K
    if (gs and gs < K) or (C > 1 and gcs < rows) or (gbs and gbs < (C - 1) * gcs + rows):
        m = m.contiguous()
        gs, gcs, gbs = strides(m)
    return m, gs, gcs, gbs


def _stft_beamform_istft(torch, params, x, weights, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table, check,
                         device_call, table_call):
    """What the two beamformer calls share after their refusals: the input checks on one signal's channels (check: _fft_input or
    _mfft_input), the channel axis of x and of the weights, the two descriptors and the one call."""
    if table is not None:
        if not isinstance(table, ResidentTable):
            raise ValueError("table must be a ResidentTable or None")
        dev, handle = table.device, table._live()
    else:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("x must be a float32 CUDA tensor")
        dev, handle = x.device.index, None
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError("x must be (C, T) or (B, C, T)")
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    if x3.shape[0] < 1:
        raise ValueError("zero signals")
    n_fft, L, _, C, T, frames, d = _stft_front(torch, params, x3[0], n_fft, hop, win_length, center, pad_mode, False, dev, check)
    if not center and L < n_fft:
        raise ValueError("center=False with win_length < n_fft: the first outputs have no window under them")
    nb = x3.shape[0]
    xcs = x3.stride(1) if C > 1 else T
    if (T > 1 and x3.stride(2) != 1) or (C > 1 and xcs < T) or (nb > 1 and x3.stride(0) < (C - 1) * xcs + T):
        x3 = x3.contiguous()
        xcs = T
    K = n_fft // 2 + 1
    g, gs, gcs, gbs = _beam_gains(torch, weights, nb, C, frames, K, dev)
    length = T if length is None else int(length)
    if length < 0:
        raise ValueError(f"length {length} < 0")
    out = _stft_out(torch, out, (nb, length) if x.dim() == 3 else (length,), x, "x")
    shift = params.dat_width - 1 if shift is None else int(shift)
    sa = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                     x_stride=x3.stride(0) if nb > 1 else 0)
    ss = B.make_stft(nb, length, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], shift=shift)
    tail = (ctypes.byref(sa), ctypes.byref(ss), B.OLA_NORMALIZE if normalize else 0, ctypes.c_void_p(x3.data_ptr()), C, xcs,
            ctypes.c_void_p(g.data_ptr()), gs, gcs, gbs, ctypes.c_void_p(out.data_ptr()))
    if handle is None:
        B.check(getattr(B.lib(), device_call)(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(getattr(B.lib(), table_call)(handle, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def stft_beamform_istft(params, x, weights, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                        shift=None, out=None, table=None):
    """A filter-and-sum beamformer (delay-and-sum, MVDR, GEV, ...) over C channels in ONE launch (bhw_beam_fft_f32_device): stft() of
    every channel, a complex weight per channel and bin, the sum over the channels in the frequency domain and ONE istft() -- C forward
    transforms and one inverse per output frame, no spectrum in memory.  x (C, T) or (B, C, T), float32, 1 <= C <= 64; weights
    complex64 (C, K), (C, F, K) or (1 | B, C, 1 | F, K), K = n_fft // 2 + 1, F the frames stft() gives, the last axis contiguous.  A
    batch or frame axis of size 1 or stride 0 (an expand() view) is never materialised; a conjugate view is resolved first; a
    broadcast CHANNEL axis raises (the same weights on every channel are x.sum(-2) and stft_cmask_istft).  Returns float32
    (B, length), or (length,) for 2-D x; length defaults to T.  With Y_c = bhw.stft(params, x[..., c, :], n_fft, hop, ...) and
    G_c = weights[..., c, :, :], in separate float32 operations,

        P_c.real = Y_c.real * G_c.real - Y_c.imag * G_c.imag        P_c.imag = Y_c.real * G_c.imag + Y_c.imag * G_c.real

    -- stft_cmask_istft()'s formula -- and Z = P_0, then Z = Z + P_c for c = 1 .. C - 1 per part, in that order.  The result equals
    bhw.istft(params, Z, n_fft, hop, ..., length=length, normalize=normalize) BIT FOR BIT: what eager float32 torch operations on the
    two planes give in a Python loop over the channels.  The weights are applied as given: for w^H x pass w.conj().  Bins 0 and
    n_fft / 2 behave per channel as in stft_cmask_istft(); with C = 1 the call equals stft_cmask_istft() bit for bit.  n_fft: a power
    of two in 16..2048.  ValueError naming what takes it, before any device is asked for: real weights, complex x (the I/Q beamformer
    is not built: stft_cmask_istft_iq per channel and a sum), a mixed-radix n_fft (stft_beamform_istft_mixed), 4096 (stft, the weights
    and a sum, istft).  `out`, `table` and the other keywords are stft_cmask_istft()'s (bhw_beam_fft_f32_from_table)."""
    import torch as host_torch                            # the refusals look at no device: they come before _torch() asks for one
    _beam_refusals(host_torch, x, weights, n_fft, False)
    torch = _torch()
    return _stft_beamform_istft(torch, params, x, weights, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                                _fft_input, "bhw_beam_fft_f32_device", "bhw_beam_fft_f32_from_table")


def stft_beamform_istft_mixed(params, x, weights, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None,
                              normalize=True, shift=None, out=None, table=None):
    """stft_beamform_istft() at the n_fft of stft_mixed() in ONE launch (bhw_beam_mfft_f32_device): n_fft even, 2^a·3^b·5^c, no power
    of two, from 18 to 2000 -- 320, 400, 480, 960, 1000, 1200, 1920.  The arguments, the layouts of x and of the weights, the formula
    and the order of the sum are stft_beamform_istft()'s, with stft_mixed() and istft_mixed() as the transforms: the result equals
    istft_mixed() of the summed rows BIT FOR BIT, and stft_cmask_istft_mixed() at C = 1.  ValueError naming what takes it: real
    weights, complex x (stft_cmask_istft_iq_mixed per channel and a sum), a power of two (stft_beamform_istft), an n_fft of 2048 or
    more (stft_mixed, the weights and a sum, istft_mixed).  `table`: bhw_beam_mfft_f32_from_table."""
    import torch as host_torch
    _beam_refusals(host_torch, x, weights, n_fft, True)
    torch = _torch()
    return _stft_beamform_istft(torch, params, x, weights, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                                _mfft_input, "bhw_beam_mfft_f32_device", "bhw_beam_mfft_f32_from_table")


# ---- the same for I/Q input: a real or complex gain on every one of the n_fft bins ---------------------------------------------------------

def _mask_iq_refusals(torch, x, mask, n_fft, complex_gains, mixed):
    """What the four I/Q mask calls do not take, refused naming the call that does, before any check that needs a device."""
    c, tail = ("c" if complex_gains else ""), ("_mixed" if mixed else "")
    name = f"bhw.stft_{c}mask_istft_iq{tail}"
    if isinstance(x, torch.Tensor) and not x.is_complex():
        raise ValueError(f"{name} takes complex64 (I/Q) input, got {x.dtype}: bhw.stft_{c}mask_istft{tail} takes a real signal")
    if isinstance(mask, torch.Tensor) and mask.is_complex() != complex_gains:
        other = f"bhw.stft_{'' if complex_gains else 'c'}mask_istft_iq{tail}"
        raise ValueError(f"{name} takes {'complex64' if complex_gains else 'real float32'} gains, got {mask.dtype}: {other} takes "
                         f"{'real' if complex_gains else 'complex'} gains")
    n = int(n_fft)
    if mixed and B.cfft_supported(n):
        raise ValueError(f"n_fft {n} is a power of two: bhw.stft_{c}mask_istft_iq takes it (one transform per n_fft)")
    if not mixed and B.cmfft_supported(n):
        raise ValueError(f"{name} takes n_fft a power of two in {B.CFFT_MIN_N}..{B.CFFT_MAX_N}, got {n} (a mixed-radix n_fft: "
                         f"bhw.stft_{c}mask_istft_iq_mixed takes it)")
    if n > B.CFFT_MAX_N and (B.fft_supported(n) or B.mfft_supported(n)):
        raise ValueError(f"{name} takes n_fft up to {B.CFFT_MAX_N if not mixed else B.CMFFT_MAX_N}, got {n}: no fused I/Q transform takes it "
                         f"(the three-call route there is stft_frames, torch.fft.fft, a multiply, torch.fft.ifft and istft_overlap_add)")


def _stft_mask_istft_iq(params, iq, gains, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, fftshift, out, table,
                        complex_gains, mixed):
    """The four I/Q calls: their refusals, then _stft_mask_istft with the I/Q input check, K = n_fft and the shift of the gain columns."""
    import torch as host_torch                            # the refusals look at no device: they come before _torch() asks for one
    _mask_iq_refusals(host_torch, iq, gains, n_fft, complex_gains, mixed)
    torch = _torch()
    name = f"bhw_{'c' if complex_gains else ''}mask_{'cmfft' if mixed else 'cfft'}_f32"
    return _stft_mask_istft(torch, params, iq, gains, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, out, table,
                            _cmfft_input if mixed else _cfft_input, name + "_device", name + "_from_table", complex_gains, True, fftshift)


def stft_mask_istft_iq(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                       shift=None, fftshift=False, out=None, table=None):
    """stft_mask_istft() for complex baseband in ONE launch (bhw_mask_cfft_f32_device): stft_iq(), a real gain on every bin and
    istft_iq() with neither spectrum in memory -- interference excision, notch and blanking masks.  x (T,) or (B, T), complex64; mask
    real float32 (K,), (F, K) or (1 | B, 1 | F, K) with K = n_fft (all bins, not n_fft // 2 + 1), the last axis contiguous; an axis
    of size 1 or stride 0 (an expand() view) is never materialised.  fftshift=True: the gain of bin k is mask column
    (k + n_fft // 2) % n_fft, the column stft_iq(fftshift=True) writes bin k to -- the mask is torch.fft.fftshift(g, dim=-1) of the
    gains g in natural order, so a mask designed on a centred frequency axis is passed as it is; x and the result are not touched by
    it.  Returns complex64 (B, length), or (length,) for 1-D x; length defaults to T.  With Y = bhw.stft_iq(params, x, n_fft, hop, ...)
    in natural bin order and g the gains in that order, the result equals

        bhw.istft_iq(params, torch.complex(Y.real * g, Y.imag * g), n_fft, hop, ..., length=length, normalize=normalize)

    BIT FOR BIT.  n_fft: a power of two in 16..2048.  ValueError naming the call that takes the input: a real x (stft_mask_istft), a
    complex mask (stft_cmask_istft_iq), a mixed-radix n_fft (stft_mask_istft_iq_mixed).  center=False with win_length < n_fft is
    refused, and there is no detrending (it has no inverse).  `out`: a contiguous complex64 tensor of the returned shape that shares
    no memory with x or mask.  `table`: a ResidentTable of these params (bhw_mask_cfft_f32_from_table), or None."""
    return _stft_mask_istft_iq(params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, fftshift, out, table,
                               False, False)


def stft_cmask_istft_iq(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                        shift=None, fftshift=False, out=None, table=None):
    """stft_mask_istft_iq() with a COMPLEX gain per bin (bhw_cmask_cfft_f32_device): an equaliser or channeliser response H[k] as one
    (K,) row, a fractional delay, per-channel beamforming weights (B, 1, K).  mask complex64, K = n_fft; a conjugate view is resolved
    first.  With Y = bhw.stft_iq(...) and G the gains in natural bin order the masked spectrum is, in separate float32 operations,

        Z.real = Y.real * G.real - Y.imag * G.imag        Z.imag = Y.real * G.imag + Y.imag * G.real

    and the result equals bhw.istft_iq(params, Z, ...) BIT FOR BIT; equality with torch's complex Y * G is not promised.  No bin is
    special: bins 0 and n_fft / 2 of a complex signal carry an imaginary part and G.imag acts on them like on any other bin.
    ValueError: a real mask names stft_mask_istft_iq, a real x stft_cmask_istft, a mixed-radix n_fft stft_cmask_istft_iq_mixed."""
    return _stft_mask_istft_iq(params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, fftshift, out, table,
                               True, False)


def stft_mask_istft_iq_mixed(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                             shift=None, fftshift=False, out=None, table=None):
    """stft_mask_istft_iq() at the n_fft of stft_iq_mixed() (bhw_mask_cmfft_f32_device): the 91 sizes 2^a·3^b·5^c in 18..2025 that are
    no power of two, odd ones included.  The result equals istft_iq_mixed() of the gained stft_iq_mixed() rows BIT FOR BIT;
    fftshift=True uses integer division at an odd n_fft too.  A power of two names stft_mask_istft_iq."""
    return _stft_mask_istft_iq(params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, fftshift, out, table,
                               False, True)


def stft_cmask_istft_iq_mixed(params, x, mask, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", length=None, normalize=True,
                              shift=None, fftshift=False, out=None, table=None):
    """stft_cmask_istft_iq() at the n_fft of stft_iq_mixed() (bhw_cmask_cmfft_f32_device); the formula, the layouts and the errors are
    stft_cmask_istft_iq()'s with stft_iq_mixed() and istft_iq_mixed() as the two transforms: the result equals istft_iq_mixed() of the
    masked stft_iq_mixed() rows BIT FOR BIT.  A power of two names stft_cmask_istft_iq."""
    return _stft_mask_istft_iq(params, x, mask, n_fft, hop, win_length, center, pad_mode, length, normalize, shift, fftshift, out, table,
                               True, True)


def fbank_bands(weights):
    """The sparse form of a dense (K, filters) bank, on the host: (first, offset, weight) as numpy uint32, uint32 and float32 arrays.
    Filter m's band runs from its first to its last nonzero weight (interior zeros are kept as weights) and owns
    weight[offset[m] : offset[m + 1]], which multiplies the bins first[m], first[m] + 1, ...; an all-zero filter has an empty band
    (first 0).  -0.0 counts as zero."""
    import numpy as np
    w = np.asarray(weights)
    if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError("a filter bank is a dense (bins, filters) array")
    if w.dtype.kind not in "fiu":
        raise ValueError(f"a filter bank holds real weights, got {w.dtype}")
    w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError("a filter bank's weights must be finite")
    K, M = w.shape
    first = np.zeros(M, dtype=np.uint32)
    offset = np.zeros(M + 1, dtype=np.uint32)
    parts = []
    for m in range(M):
        nz = np.flatnonzero(w[:, m])
        if nz.size:
            first[m] = nz[0]
            parts.append(w[nz[0]:nz[-1] + 1, m])
            offset[m + 1] = offset[m] + (nz[-1] + 1 - nz[0])
        else:
            offset[m + 1] = offset[m]
    weight = np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)
    return first, offset, np.ascontiguousarray(weight, dtype=np.float32)


def fbank_dense(first, offset, weight, bins):
    """The dense (bins, filters) float32 array of a sparse bank (the inverse of fbank_bands), on the host."""
    import numpy as np
    M = len(first)
    w = np.zeros((int(bins), M), dtype=np.float32)
    for m in range(M):
        c = int(offset[m + 1]) - int(offset[m])
        w[int(first[m]):int(first[m]) + c, m] = weight[int(offset[m]):int(offset[m + 1])]
    return w


class FilterBank:
    """A filter bank for spectrogram(), built ONCE from a dense (K, filters) float array or tensor -- the layout of
    torchaudio.functional.melscale_fbanks and of mel_weights() -- and kept on `device` in the sparse form of bhw_fbank: per filter
    the band from its first to its last nonzero weight (interior zeros kept, an all-zero filter empty).  The contents are validated
    here, so a call never hands the kernel an inconsistent bank; the upload (and its one synchronisation, when the weights come from
    a device tensor) happens here and never in spectrogram().  filters, bins, weights: the counts; dense(): the (K, filters) float32
    numpy array the bank stands for."""

    MAX_FILTERS, MAX_WEIGHTS = 4096, 1 << 24

    def __init__(self, weights, device=None):
        import numpy as np
        torch = _torch()
        if isinstance(weights, torch.Tensor):
            if device is None and weights.is_cuda:
                device = weights.device
            weights = weights.detach().cpu().numpy()
        first, offset, weight = fbank_bands(weights)
        K, M = np.asarray(weights).shape
        if M > self.MAX_FILTERS:
            raise ValueError(f"{M} filters: a bank holds 1..{self.MAX_FILTERS}")
        if weight.size > self.MAX_WEIGHTS:
            raise ValueError(f"{weight.size} weights: a bank holds 2^24 at most")
        assert offset[0] == 0 and offset[-1] == weight.size and (np.diff(offset.astype(np.int64)) >= 0).all()
        assert ((first.astype(np.int64) + np.diff(offset.astype(np.int64))) <= K).all()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("a FilterBank lives on a CUDA device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.filters, self.bins, self.weights = int(M), int(K), int(weight.size)
        self._host = (first, offset, weight)
        # uint32 words travel as int32 tensors of the same bits
        self._first = torch.from_numpy(first.view(np.int32)).to(dev)
        self._offset = torch.from_numpy(offset.view(np.int32)).to(dev)
        self._weight = torch.from_numpy(weight if weight.size else np.zeros(1, dtype=np.float32)).to(dev)
        self.descriptor = B.make_fbank(M, K, weight.size, self._first.data_ptr(), self._offset.data_ptr(), self._weight.data_ptr())

    def dense(self):
        return fbank_dense(*self._host, self.bins)

    def __repr__(self):
        return f"FilterBank(filters={self.filters}, bins={self.bins}, weights={self.weights}, device={self.device})"


def mel_weights(n_fft, n_mels, sample_rate, *, f_min=0.0, f_max=None, norm=None, mel_scale="htk"):
    """The mel filter bank of torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate, norm,
    mel_scale), restated: a host numpy float32 array (K, n_mels), K = n_fft // 2 + 1, computed in float64 and rounded once.
    all_freqs = linspace(0, sample_rate // 2, K); n_mels + 2 points equally spaced in mel between f_min and f_max (default
    sample_rate / 2); filter m is the triangle max(0, min(up, down)) over points m, m + 1, m + 2; norm="slaney" scales filter m by
    2 / (f[m + 2] - f[m]).  mel_scale: "htk" (2595 log10(1 + f / 700)) or "slaney" (linear below 1 kHz, logarithmic above).
    FilterBank(mel_weights(...), device=...) is the mel bank of spectrogram()."""
    import numpy as np
    n_fft, n_mels = int(n_fft), int(n_mels)
    if n_fft < 2 or n_mels < 1:
        raise ValueError("n_fft must be >= 2 and n_mels >= 1")
    if mel_scale not in ("htk", "slaney"):
        raise ValueError(f"mel_scale must be 'htk' or 'slaney', got {mel_scale!r}")
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', got {norm!r}")
    f_max = float(sample_rate) / 2 if f_max is None else float(f_max)
    f_min = float(f_min)
    if not 0.0 <= f_min < f_max:
        raise ValueError(f"need 0 <= f_min < f_max, got {f_min}, {f_max}")
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def to_mel(f):
        if mel_scale == "htk":
            return 2595.0 * np.log10(1.0 + f / 700.0)
        return f / f_sp if f < min_log_hz else min_log_mel + np.log(f / min_log_hz) / logstep

    def to_hz(m):
        if mel_scale == "htk":
            return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    K = n_fft // 2 + 1
    all_freqs = np.linspace(0.0, float(int(sample_rate) // 2), K)
    f_pts = to_hz(np.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2))
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    return np.ascontiguousarray(fb, dtype=np.float32)


def _spectrogram(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, fbank, shift, out, dev, table):
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev)
    K = n_fft // 2 + 1
    if fbank is not None:
        if not isinstance(fbank, FilterBank):
            raise ValueError("fbank must be a FilterBank (FilterBank(dense_weights, device=...)) or None")
        if fbank.bins != K:
            raise ValueError(f"the filter bank has {fbank.bins} bins, n_fft // 2 + 1 is {K}")
        if fbank.device != x.device:
            raise ValueError(f"the filter bank is on {fbank.device}, x on {x.device}")
    W = K if fbank is None else fbank.filters
    out, ys, ybs = _fft_out(torch, out, (nb, frames, W) if x.dim() == 2 else (frames, W), x, torch.float32)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                    x_stride=xb.stride(0) if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    tail = (ctypes.byref(s), B.WELCH_DETREND_CONSTANT if detrend else 0, ctypes.byref(fbank.descriptor) if fbank is not None else None,
            ctypes.c_void_p(xb.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_spectrogram_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(B.lib().bhw_spectrogram_f32_from_table(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def spectrogram(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, fbank=None, shift=None,
                out=None):
    """The power spectrogram of a batch, or its filter-bank (mel) spectrogram, in ONE launch (bhw_spectrogram_f32_device): x (T,) or
    (B, T), real float32, framed, windowed and transformed exactly as stft() does (same arguments), and each bin written as
    fl32(re^2 + im^2) of the float32 pair stft() would have written -- bit for bit -- so the complex spectrum never reaches memory.
    With fbank (a FilterBank, e.g. FilterBank(mel_weights(n_fft, 80, 16000), device=x.device)) the powers stay in the kernel too
    and each row is folded through the bank: column m is the binary64 sum, in ascending bin order, of power * weight over filter
    m's band, rounded once to float32.  Returns float32 (B, F, W) or (F, W) for 1-D x, W = n_fft // 2 + 1 or fbank.filters;
    `.transpose(-1, -2)` gives torchaudio's (..., freq, time) layout.  log, magnitude and a complex output next to the power are
    not built: apply torch.log to the small result.  n_fft: a power of two in 16..4096 (ValueError otherwise; complex x too).
    `out`: float32 of the returned shape, columns contiguous, rows and signals apart (its gaps are left alone)."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _spectrogram(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, fbank, shift, out, x.device.index, None)


# ---- mixed-radix fused window and real FFT: n_fft like 400, 480, 960, 1000 -----------------------------------------------------------------

def _mfft_input(torch, x, n_fft, dev):
    """_fft_input for the mixed-radix calls: real float32 (T,) or (B, T) on `dev`, n_fft one the mixed-radix kernel takes."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a float32 CUDA tensor on the call's device")
    if x.dtype != torch.float32:
        raise ValueError(f"the fused FFT takes real float32 input, got {x.dtype} (complex input: stft_frames + torch.fft)")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    n = int(n_fft)
    if n > 0 and n & (n - 1) == 0:
        raise ValueError(f"n_fft {n} is a power of two: bhw.stft / bhw.spectrogram transform it (one transform per n_fft)")
    if not B.mfft_supported(n):
        raise ValueError(f"the mixed-radix fused FFT takes n_fft even 2^a·3^b·5^c in {B.MFFT_MIN_N}..{B.MFFT_MAX_N}, got {n}")


def _stft_mixed(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, power, fbank, shift, out, dev, table):
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev, _mfft_input)
    K = n_fft // 2 + 1
    if fbank is not None:
        if not isinstance(fbank, FilterBank):
            raise ValueError("fbank must be a FilterBank (FilterBank(dense_weights, device=...)) or None")
        if fbank.bins != K:
            raise ValueError(f"the filter bank has {fbank.bins} bins, n_fft // 2 + 1 is {K}")
        if fbank.device != x.device:
            raise ValueError(f"the filter bank is on {fbank.device}, x on {x.device}")
    W = K if fbank is None else fbank.filters
    out, ys, ybs = _fft_out(torch, out, (nb, frames, W) if x.dim() == 2 else (frames, W), x, torch.float32 if power else torch.complex64)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                    x_stride=xb.stride(0) if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    flags = (B.WELCH_DETREND_CONSTANT if detrend else 0) | (B.MFFT_POWER if power else 0)
    tail = (ctypes.byref(s), flags, ctypes.byref(fbank.descriptor) if fbank is not None else None, ctypes.c_void_p(xb.data_ptr()),
            ctypes.c_void_p(out.data_ptr()))
    if table is None:
        B.check(B.lib().bhw_stft_mfft_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(B.lib().bhw_stft_mfft_f32_from_table(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def stft_mixed(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, out=None):
    """stft() for the row lengths speech and audio code uses and a power-of-two transform refuses, in ONE launch
    (bhw_stft_mfft_f32_device): n_fft even, 2^a·3^b·5^c, in 16..4095 and not a power of two -- 400 (torchaudio's and Whisper's
    default), 480, 960, 1000, 1200, 1920.  The arguments, the shapes, the `out` rules and the errors are stft()'s: x (T,) or (B, T),
    real float32, framed and windowed exactly as stft_frames() / welch_frames() do (their rows bit for bit) and transformed in the
    same kernel by a float32 mixed-radix FFT in LDS (radix-5, -3, -4 and -2 Stockham passes).  Returns complex64 (B, F, K) or (F, K),
    K = n_fft // 2 + 1; `stft_mixed(p, x, 400, 160).transpose(-1, -2)` is the layout of torch.stft(x, 400, 160, window=v,
    return_complex=True).  detrend=True (needs center=False) forms scipy's Welch segments, and
    welch_psd(stft_mixed(..., detrend=True, center=False), scale, nfft=n_fft) is the fused Welch estimate at such an nfft.  A
    power-of-two n_fft raises ValueError (bhw.stft transforms it: one transform per n_fft); any other unsupported n_fft raises
    ValueError too.  The FFT is accurate to a float32 FFT's error, not pinned bit for bit."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _stft_mixed(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, False, None, shift, out, x.device.index, None)


def spectrogram_mixed(params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, fbank=None, shift=None,
                      out=None):
    """spectrogram() at the n_fft of stft_mixed() (bhw_stft_mfft_f32_device with BHW_MFFT_POWER): each bin fl32(re^2 + im^2), taken in
    binary64, of the float32 pair stft_mixed() would have written -- bit for bit -- or, with fbank (a FilterBank of n_fft // 2 + 1
    bins, e.g. FilterBank(mel_weights(400, 80, 16000), device=x.device): Whisper's 400 / 160 / 80 mel front end), those powers folded
    through the bank exactly as spectrogram() folds them.  Returns float32 (B, F, W) or (F, W), W = n_fft // 2 + 1 or fbank.filters.
    The arguments, `out` rules and errors are spectrogram()'s; a power-of-two n_fft raises ValueError (bhw.spectrogram transforms
    it)."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _stft_mixed(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, True, fbank, shift, out, x.device.index, None)


# ---- fused log spectrogram, log-mel spectrogram and MFCC ------------------------------------------------------------------------------------

def dct_weights(n_coeffs, n_mels, norm="ortho"):
    """The DCT-II matrix of torchaudio.functional.create_dct(n_mfcc, n_mels, norm), restated: a host numpy float32 array
    (n_mels, n_coeffs) computed in float64 and rounded once.  Entry (m, j) is cos(pi / n_mels * (m + 0.5) * j), times 2 for norm
    None; for norm "ortho" column 0 is scaled by 1 / sqrt(2) and everything by sqrt(2 / n_mels).  DctMatrix(dct_weights(13, 80),
    device=...) is the DCT of mfcc()."""
    import numpy as np
    n_coeffs, n_mels = int(n_coeffs), int(n_mels)
    if n_coeffs < 1 or n_mels < 1:
        raise ValueError("n_coeffs and n_mels must be >= 1")
    if norm not in (None, "ortho"):
        raise ValueError(f"norm must be None or 'ortho', got {norm!r}")
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    j = np.arange(n_coeffs, dtype=np.float64)[None, :]
    d = np.cos(np.pi / n_mels * (m + 0.5) * j)
    if norm is None:
        d = d * 2.0
    else:
        d[:, 0] *= 1.0 / np.sqrt(2.0)
        d = d * np.sqrt(2.0 / n_mels)
    return np.ascontiguousarray(d, dtype=np.float32)


class DctMatrix:
    """A dense matrix for the DCT stage of mfcc() / log_spectrogram(dct=), built ONCE from a (filters, coeffs) float array or tensor --
    the layout of torchaudio.functional.create_dct and of dct_weights() -- and kept on `device` row-major.  The contents are
    validated here, and the upload (and its one synchronisation, when the matrix comes from a device tensor) happens here and never
    in the call.  filters, coeffs: the shape; dense(): the (filters, coeffs) float32 numpy array."""

    MAX_COEFFS, MAX_WORDS = B.LOG_MAX_COEFFS, B.LOG_MAX_DCT

    def __init__(self, dense, device=None):
        import numpy as np
        torch = _torch()
        if isinstance(dense, torch.Tensor):
            if device is None and dense.is_cuda:
                device = dense.device
            dense = dense.detach().cpu().numpy()
        d = np.asarray(dense)
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 1:
            raise ValueError("a DCT matrix is a dense (filters, coeffs) array")
        if d.dtype.kind not in "fiu":
            raise ValueError(f"a DCT matrix holds real numbers, got {d.dtype}")
        d = np.array(d, dtype=np.float32, order="C")                 # a copy: the caller's array may change or be read-only
        if not np.isfinite(d).all():
            raise ValueError("a DCT matrix's entries must be finite")
        M, C = d.shape
        if C > self.MAX_COEFFS:
            raise ValueError(f"{C} coefficients: a DCT matrix holds 1..{self.MAX_COEFFS}")
        if M * C > self.MAX_WORDS:
            raise ValueError(f"{M * C} entries: a DCT matrix holds 2^24 at most")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("a DctMatrix lives on a CUDA device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.filters, self.coeffs = int(M), int(C)
        self._host = d
        self._dev = torch.from_numpy(d).to(dev)

    def data_ptr(self):
        return self._dev.data_ptr()

    def dense(self):
        return self._host.copy()

    def __repr__(self):
        return f"DctMatrix(filters={self.filters}, coeffs={self.coeffs}, device={self.device})"


_LOG_MULT = {"ln": 1.0, "log10": 1.0 / math.log(10.0), "db": 10.0 / math.log(10.0)}


def log_multiplier(log):
    """The multiplier of the natural log that `log` names: "db" (10 / ln 10, the dB of a power), "ln" (1), "log10" (1 / ln 10), or a
    finite non-zero float."""
    if isinstance(log, str):
        if log not in _LOG_MULT:
            raise ValueError(f"log must be 'db', 'ln', 'log10' or a float multiplier of ln, got {log!r}")
        return _LOG_MULT[log]
    if isinstance(log, bool) or not isinstance(log, (int, float)) or not math.isfinite(log) or log == 0:
        raise ValueError(f"log must be 'db', 'ln', 'log10' or a finite non-zero float multiplier of ln, got {log!r}")
    return float(log)


def _logspec_input(mixed):
    """_fft_input / _mfft_input under the names of the log calls: complex x first, then the other family's n_fft by name."""
    def check(torch, x, n_fft, dev):
        if isinstance(x, torch.Tensor) and x.is_complex():
            raise ValueError(f"the fused log spectrogram takes real input, got {x.dtype} (I/Q input is not built)")
        n = int(n_fft)
        if mixed and n > 0 and n & (n - 1) == 0:
            raise ValueError(f"n_fft {n} is a power of two: bhw.log_spectrogram / bhw.mfcc transform it (one transform per n_fft)")
        if not mixed and B.mfft_supported(n):
            raise ValueError(f"n_fft {n} is no power of two: bhw.log_spectrogram_mixed / bhw.mfcc_mixed transform it "
                             "(one transform per n_fft)")
        (_mfft_input if mixed else _fft_input)(torch, x, n_fft, dev)
    return check


def _logspec(torch, mixed, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, dev, table):
    mult = log_multiplier(log)
    floor = float(floor)
    if not math.isfinite(floor) or floor <= 0:
        raise ValueError(f"floor must be finite and > 0, got {floor!r}")
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev,
                                                 _logspec_input(mixed))
    K = n_fft // 2 + 1
    if fbank is not None:
        if not isinstance(fbank, FilterBank):
            raise ValueError("fbank must be a FilterBank (FilterBank(dense_weights, device=...)) or None")
        if fbank.bins != K:
            raise ValueError(f"the filter bank has {fbank.bins} bins, n_fft // 2 + 1 is {K}")
        if fbank.device != x.device:
            raise ValueError(f"the filter bank is on {fbank.device}, x on {x.device}")
    W = K if fbank is None else fbank.filters
    if dct is not None:
        if not isinstance(dct, DctMatrix):
            raise ValueError("dct must be a DctMatrix (DctMatrix(dense, device=...)) or None")
        if fbank is None:
            raise ValueError("a DCT takes the rows of a filter bank: pass fbank")
        if dct.filters != fbank.filters:
            raise ValueError(f"the DCT matrix has {dct.filters} rows, the filter bank {fbank.filters} filters")
        if dct.device != x.device:
            raise ValueError(f"the DCT matrix is on {dct.device}, x on {x.device}")
        if fbank.filters > n_fft:
            raise ValueError(f"{fbank.filters} filters above n_fft {n_fft}: the DCT stage holds the log row in n_fft floats")
        W = dct.coeffs
    out, ys, ybs = _fft_out(torch, out, (nb, frames, W) if x.dim() == 2 else (frames, W), x, torch.float32)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                    x_stride=xb.stride(0) if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    ls = B.make_logspec(floor, mult, add=add) if dct is None else \
        B.make_logspec(floor, mult, add=add, coeffs=dct.coeffs, dct_rows=dct.filters, d_dct=dct.data_ptr())
    tail = (ctypes.byref(s), B.WELCH_DETREND_CONSTANT if detrend else 0, ctypes.byref(fbank.descriptor) if fbank is not None else None,
            ctypes.byref(ls), ctypes.c_void_p(xb.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    L_ = B.lib()
    device_call, table_call = (L_.bhw_logspec_mfft_f32_device, L_.bhw_logspec_mfft_f32_from_table) if mixed else \
        (L_.bhw_logspec_f32_device, L_.bhw_logspec_f32_from_table)
    if table is None:
        B.check(device_call(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(table_call(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def _logspec_front(mixed, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, table):
    """The library form (table None: the coefficients by direct CORDIC) or the form that gathers them from `table`, a ResidentTable
    (bhw_logspec*_f32_from_table: no allocation by the library, no synchronisation, capturable into a graph on its first call)."""
    torch = _torch()
    if table is not None:
        if not isinstance(table, ResidentTable):
            raise ValueError("table must be a ResidentTable or None")
        return _logspec(torch, mixed, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift,
                        out, table.device, table._live())
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _logspec(torch, mixed, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out,
                    x.device.index, None)


def _mfcc_args(fbank, dct):
    if fbank is None or dct is None:
        raise ValueError("mfcc takes fbank (a FilterBank) and dct (a DctMatrix)")


def log_spectrogram(params, x, n_fft, hop, *, fbank=None, log="db", floor=1e-10, add=False, dct=None, win_length=None, center=True,
                    pad_mode="reflect", detrend=False, shift=None, out=None, table=None):
    """The dB / log spectrogram, the log-mel spectrogram or (with dct) the MFCCs of a batch in ONE launch (bhw_logspec_f32_device):
    x, the framing, the window, the transform and the bank are spectrogram()'s, and each word q that call would have written leaves
    the kernel as fl32(mult * ln(max(q, floor))) -- or ln(q + floor) with add=True -- taken in binary64.  log: "db" (10 log10), "ln",
    "log10" or a float multiplier of ln.  With dct (a DctMatrix of fbank.filters rows; needs fbank, filters <= n_fft) the log row is
    folded through it in binary64, in ascending filter order, rounded once: W = dct.coeffs columns.  Returns float32 (B, F, W) or
    (F, W), W = n_fft // 2 + 1, fbank.filters or dct.coeffs.  The log words are within one float32 ulp of the binary64 formula; given
    them the DCT is exact.  top_db, Whisper's max - 8 clamp, magnitude, liftering and deltas are not built: apply them to the small
    result.  n_fft: a power of two in 16..4096 (a mixed-radix n_fft raises ValueError naming log_spectrogram_mixed; complex x too).
    `out`: as spectrogram().  `table`: a ResidentTable of these params to gather the window coefficients from
    (bhw_logspec_f32_from_table: no allocation by the library, no synchronisation, capturable on its first call), or None."""
    return _logspec_front(False, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, table)


def log_spectrogram_mixed(params, x, n_fft, hop, *, fbank=None, log="db", floor=1e-10, add=False, dct=None, win_length=None, center=True,
                          pad_mode="reflect", detrend=False, shift=None, out=None, table=None):
    """log_spectrogram() at the n_fft of stft_mixed() (bhw_logspec_mfft_f32_device): the words of spectrogram_mixed() through the same
    log and DCT stages.  log_spectrogram_mixed(p, x, 400, 160, fbank=FilterBank(mel_weights(400, 80, 16000)), log="log10") is
    Whisper's log-mel front end before its clamp.  A power-of-two n_fft raises ValueError (bhw.log_spectrogram transforms it)."""
    return _logspec_front(True, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, table)


def mfcc(params, x, n_fft, hop, *, fbank, dct, log="db", floor=1e-10, add=False, win_length=None, center=True, pad_mode="reflect",
         detrend=False, shift=None, out=None, table=None):
    """log_spectrogram() with fbank and dct required: the MFCCs of a batch in ONE launch, float32 (B, F, dct.coeffs)."""
    _mfcc_args(fbank, dct)
    return _logspec_front(False, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, table)


def mfcc_mixed(params, x, n_fft, hop, *, fbank, dct, log="db", floor=1e-10, add=False, win_length=None, center=True, pad_mode="reflect",
               detrend=False, shift=None, out=None, table=None):
    """mfcc() at the n_fft of stft_mixed().  mfcc_mixed(p, x, 400, 160, fbank=FilterBank(mel_weights(400, 80, 16000)),
    dct=DctMatrix(dct_weights(13, 80)), log="ln", floor=1e-6, add=True) is torchaudio's MFCC(log_mels=True) in one launch."""
    _mfcc_args(fbank, dct)
    return _logspec_front(True, params, x, n_fft, hop, fbank, log, floor, add, dct, win_length, center, pad_mode, detrend, shift, out, table)


def _welch_fft(torch, params, x, length, hop, nfft, detrend, shift, out, dev, table):
    """The one-sided spectra of the Welch segments of x by the fused kernel: (B, frames, K) or (frames, K) complex64, into `out`
    (a packed complex64 tensor of that shape) when given."""
    L, hop = int(length), int(hop)
    nfft = L if nfft is None else int(nfft)
    _fft_input(torch, x, nfft, dev)
    if hop < 1:
        raise ValueError("hop must be >= 1 (noverlap < length)")
    if not 1 <= L <= 1 << params.phi_width:
        raise ValueError(f"length {L} outside 1..2^phi_width = {1 << params.phi_width}")
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    if nb < 1 or T < L:
        raise ValueError(f"zero segments: T = {T} < length = {L}" if nb else "zero signals")
    frames = 1 + (T - L) // hop
    xb = _stft_input(xb, (T,))
    K = nfft // 2 + 1
    out, ys, ybs = _fft_out(torch, out, (nb, frames, K) if x.dim() == 2 else (frames, K), x)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, hop, nfft, shift=shift, x_stride=xb.stride(0) if nb > 1 else 0, y_stride=ys, y_batch_stride=ybs)
    return _fft_launch(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0, xb, out, dev, table)


# ---- Welch's method around the FFT: window sums, detrended segments, averaged periodogram ----------------------------------------------

_SUMS_CACHE = {}        # (params bytes, length, shift, f32) -> the numbers of window_sums (library form; a ResidentTable keeps its own)


def _sums_key(params, length, shift, f32):
    return (bytes(params), int(length), int(shift), bool(f32))


def _window_sums(torch, params, length, f32, shift, dev, table, cache):
    """The numbers of window_sums, read back once per (params, length, shift, f32) and cached in `cache`."""
    length = int(length)
    shift = params.dat_width - 1 if shift is None else int(shift)
    if not 0 <= shift <= 62:
        raise ValueError("shift must be in 0..62")
    key = _sums_key(params, length, shift, f32)
    hit = cache.get(key)
    if hit is not None:
        return hit
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the window sums of this (params, length, shift) have not been read yet: call once outside the capture")
    words = torch.empty(4, dtype=torch.int64, device=f"cuda:{dev}")
    flags = B.SUMS_F32 if f32 else 0
    if table is None:
        B.check(B.lib().bhw_window_sums_device(ctypes.byref(params), length, dev, _stream_ptr(torch, dev), flags,
                                               ctypes.c_void_p(words.data_ptr())))
    else:
        B.check(B.lib().bhw_window_sums_from_table(table, ctypes.byref(params), length, _stream_ptr(torch, dev), flags,
                                                   ctypes.c_void_p(words.data_ptr())))
    w = [int(v) & ((1 << 64) - 1) for v in words.cpu().tolist()]
    res = B.sums_from_words(w, shift, length)
    cache[key] = res
    return res


def window_sums(params, length, *, f32=False, shift=None, device=None):
    """The exact sums of the window of `length` (1..2^phi_width), computed on the device without storing the window
    (bhw_window_sums_device): a dict with the Python ints s1 = sum u[k] and s2 = sum u[k]^2 (u = w, or with f32=True the integer
    fl32(w) the float calls multiply by), S1 = s1 * 2^-shift and S2 = s2 * 2^-2 shift (each rounded once to a float; shift defaults
    to dat_width - 1), coherent_gain = S1 / length and enbw_bins = length * S2 / S1^2.  Reads the four result words back (one
    synchronisation) the first time; the numbers of a (params, length, shift, f32) are cached."""
    torch = _torch()
    dev = _dev_index(torch, device)
    return _window_sums(torch, params, length, f32, shift, dev, None, _SUMS_CACHE)


def _welch_frames_call(torch, params, x, length, hop, nfft, detrend, shift, out, workspace, dev):
    """Checks and shapes of welch_frames: (bhw_stft, L, flags, the x read, out, workspace)."""
    C = _stft_float(torch, x, "x", dev)
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    L, hop = int(length), int(hop)
    nfft = L if nfft is None else int(nfft)
    if hop < 1:
        raise ValueError("hop must be >= 1 (noverlap < length)")
    if not 1 <= L <= 1 << params.phi_width:
        raise ValueError(f"length {L} outside 1..2^phi_width = {1 << params.phi_width}")
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    if nb < 1 or T < L:
        raise ValueError(f"zero segments: T = {T} < length = {L}" if nb else "zero signals")
    frames = 1 + (T - L) // hop                  # scipy: (T - noverlap) // (L - noverlap) with hop = L - noverlap
    xb = _stft_input(xb, (T,))
    out = _stft_out(torch, out, (nb, frames, nfft) if x.dim() == 2 else (frames, nfft), x, "x")
    shift = params.dat_width - 1 if shift is None else int(shift)
    flags = B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0
    s = B.make_stft(nb, T, frames, hop, nfft, channels=C, shift=shift, x_stride=xb.stride(0) * C if nb > 1 else 0)
    need = nb * frames * C if flags else 0
    if need and workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)
    elif need:
        _check_out(torch, workspace, need, "workspace", torch.float32)
    return s, L, flags, xb, out, (workspace if need else None)


def _welch_frames(torch, params, x, length, hop, nfft, detrend, shift, out, workspace, dev, table):
    s, L, flags, xr, out, ws = _welch_frames_call(torch, params, x, length, hop, nfft, detrend, shift, out, workspace, dev)
    tail = (ctypes.byref(s), flags, ctypes.c_void_p(xr.data_ptr()), ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(ws.data_ptr() if ws is not None else None), ws.numel() * 4 if ws is not None else 0)
    if table is None:
        B.check(B.lib().bhw_welch_frames_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(B.lib().bhw_welch_frames_f32_from_table(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def welch_frames(params, x, length, hop, *, nfft=None, detrend="constant", shift=None, out=None, workspace=None):
    """The segments scipy.signal.welch hands its FFT (bhw_welch_frames_f32_device): x (T,) or (B, T), float32 or complex64, cut into
    frames = 1 + (T - length) // hop segments at `hop` with no padding, each with its mean removed (detrend="constant"; the mean is a
    binary64 sum in the fixed order include/bhw.h writes down, rounded to float32) or not (detrend=False: bit for bit
    stft_frames(center=False) for nfft = length), multiplied by the window of `length` and zero-padded at the end to `nfft` (default
    length).  Returns (B, frames, nfft) or (frames, nfft) in x's dtype.  `workspace`: B * frames * C float32 for the means (allocated
    when not given; detrending only)."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 or complex64 CUDA tensor")
    return _welch_frames(torch, params, x, length, hop, nfft, detrend, shift, out, workspace, x.device.index, None)


def welch_psd(Y, scale, *, nfft, onesided=True, out=None, workspace=None):
    """The averaged periodogram (bhw_welch_psd_f32): Y complex64 (F, K) or (B, F, K), the FFT of the segments; returns float32 (K,) or
    (B, K) with P[b, k] = fl32(sum over f of |Y[b, f, k]|^2 * scale * (2 for the doubled bins of a one-sided spectrum)), the sum in
    binary64 in ascending f inside blocks of 256 frames and then over the blocks in order.  onesided: K = nfft // 2 + 1 and every bin
    but 0 (and nfft / 2 for even nfft) doubled.  Y is read in place when its bins are contiguous and its rows apart, else copied.
    `out`: float32, last axis contiguous (its gaps are left alone); `workspace`: float64, B * ceil(F / 256) * K elements when F > 256
    (allocated when not given)."""
    torch = _torch()
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda or Y.dtype != torch.complex64:
        raise ValueError("Y must be a complex64 CUDA tensor")
    if Y.dim() not in (2, 3):
        raise ValueError("Y must be (frames, bins) or (B, frames, bins)")
    dev = Y.device.index
    Yb = Y if Y.dim() == 3 else Y.unsqueeze(0)
    nb, F, K = Yb.shape
    if nb < 1 or F < 1 or K < 1:
        raise ValueError("Y has no signals, frames or bins")
    nfft = int(nfft)
    if onesided and K != nfft // 2 + 1:
        raise ValueError(f"a one-sided spectrum of nfft {nfft} has {nfft // 2 + 1} bins, Y has {K}")
    if K > nfft:
        raise ValueError(f"Y has {K} bins, more than nfft {nfft}")
    Yb = _stft_input(Yb, ((F - 1) * max(Yb.stride(1), K) + K, K))
    shape = (nb, K) if Y.dim() == 3 else (K,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=Y.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != Y.device or tuple(out.shape) != shape \
            or (K > 1 and out.stride(-1) != 1) or (out.dim() == 2 and nb > 1 and out.stride(0) < K):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on Y's device, contiguous along the bins, rows apart")
    d = B.make_psd(nb, F, K, nfft, scale, onesided=onesided, y_stride=Yb.stride(1) if F > 1 else 0,
                   y_batch_stride=Yb.stride(0) if nb > 1 else 0, p_stride=out.stride(0) if (out.dim() == 2 and nb > 1) else 0)
    need = int(B.lib().bhw_welch_psd_workspace_bytes(ctypes.byref(d))) // 8
    if need and workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=Y.device)
    elif need:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    B.check(B.lib().bhw_welch_psd_f32(dev, _stream_ptr(torch, dev), ctypes.byref(d), ctypes.c_void_p(Yb.data_ptr()),
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(workspace.data_ptr() if need else None),
                                      need * 8))
    return out


def _welch(torch, params, x, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, average, dev, table, cache,
           fft="torch"):
    fused = _fft_check(fft)
    if average != "mean":
        raise ValueError("only average='mean' is built (the median needs the periodograms kept)")
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    L = int(length)
    noverlap = L // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < L:
        raise ValueError("noverlap must be less than length")
    nfft = L if nfft is None else int(nfft)
    if fused:
        if not return_onesided:
            raise ValueError("fft='fused' gives the one-sided spectrum only (return_onesided=False: fft='torch')")
        Y = _welch_fft(torch, params, x, L, L - noverlap, nfft, detrend, shift, None, dev, table)
        sums = _window_sums(torch, params, L, True, shift, dev, table, cache)
        P = welch_psd(Y, B.welch_scale(sums, Y.shape[-2], fs, scaling), nfft=nfft, onesided=True)
        return torch.fft.rfftfreq(nfft, d=1.0 / float(fs), dtype=torch.float64, device=Y.device), P
    seg = _welch_frames(torch, params, x, L, L - noverlap, nfft, detrend, shift, None, None, dev, table)
    frames = seg.shape[-2]
    sums = _window_sums(torch, params, L, True, shift, dev, table, cache)
    scale = B.welch_scale(sums, frames, fs, scaling)
    onesided = bool(return_onesided) and not seg.is_complex()
    Y = torch.fft.rfft(seg, dim=-1) if onesided else torch.fft.fft(seg, dim=-1)
    P = welch_psd(Y, scale, nfft=nfft, onesided=onesided)
    mk = torch.fft.rfftfreq if onesided else torch.fft.fftfreq
    return mk(nfft, d=1.0 / float(fs), dtype=torch.float64, device=seg.device), P


def welch(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True, scaling="density",
          shift=None, average="mean", fft="torch"):
    """Welch's power spectral density with one of this library's windows, scipy.signal.welch's defaults as the model: x (T,) or
    (B, T), float32 (one-sided spectrum, rfft) or complex64 (two-sided, fft; return_onesided is then ignored, as scipy does), cut
    into segments of `length` overlapping by noverlap (default length // 2), detrended ("constant" or False), windowed, zero-padded
    to nfft (default length), transformed by torch.fft, and the periodograms averaged: window_sums -> welch_frames -> torch.fft ->
    welch_psd.  scaling "density": 1 / (fs * sum v^2), "spectrum": 1 / (sum v)^2, from the exact sums of the float coefficients.
    Returns (freqs float64, Pxx float32 (..., K)).  The sums of a (params, length, shift) are read from the device once and cached;
    after that one call the whole chain neither synchronises nor reads back (capturable with ResidentTable.welch, whose segments
    call needs no bhw_prepare_device).  Not built (ValueError): detrend="linear", average="median", scipy's boundary and padded.
    fft="fused": the segments and their FFT come from ONE kernel (bhw_stft_fft_f32_*, see stft()) in place of welch_frames ->
    torch.fft; welch_psd then reads the same kind of Y and keeps its bit-for-bit contract given Y.  It takes real x and nfft a power
    of two in 16..4096 (ValueError otherwise) and gives the one-sided spectrum; its FFT is accurate to a float32 FFT's error, so P
    agrees with the default route to that error, not bit for bit.  The default "torch" is the chain above, unchanged.
    Cross spectra: csd(), coherence(), transfer_function(), cross_spectra()."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 or complex64 CUDA tensor")
    dev = x.device.index
    return _welch(torch, params, x, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, average, dev, None,
                  _SUMS_CACHE, fft)


# ---- fused Welch PSD: window, FFT and the frame average in one kernel --------------------------------------------------------------------

def _welch_fft_call(torch, params, L, s, flags, xb, nb, K, scale, onesided, out, workspace, dev, table, one_d, family="fft"):
    """The output and workspace rules of the fused Welch PSD and its launch: P float32 (K,) or (B, K).  family: "fft" (a power-of-two
    n_fft, bhw_welch_fft_f32_*) or "mfft" (a mixed-radix one, bhw_welch_mfft_f32_*): the two argument lists are one."""
    shape = (K,) if one_d else (nb, K)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=xb.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != xb.device or tuple(out.shape) != shape \
            or out.stride(-1) != 1 or (out.dim() == 2 and nb > 1 and out.stride(0) < K):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on x's device, contiguous along the bins, rows apart")
    need = getattr(B, f"welch_{family}_workspace_bytes")(s) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=xb.device)
    else:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    tail = (ctypes.byref(s), flags, float(scale), B.PSD_ONESIDED if onesided else 0, ctypes.c_void_p(xb.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), out.stride(0) if (out.dim() == 2 and nb > 1) else 0, ctypes.c_void_p(workspace.data_ptr()),
            workspace.numel() * 8)
    if table is None:
        B.check(getattr(B.lib(), f"bhw_welch_{family}_f32_device")(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(getattr(B.lib(), f"bhw_welch_{family}_f32_from_table")(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def _welch_fft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift, out, workspace,
                   dev, table, family="fft", hold=None):
    """hold: None (the mean: welch_fft*), or (traces, out_max, out_min) for hold_fft*: the same front and descriptor, and _hold_call
    in place of _welch_fft_call."""
    check = _fft_input if family == "fft" else _welch_mfft_input
    if hold is not None:
        B.hold_traces(hold[0])
        check = _hold_fft_input if family == "fft" else _hold_mfft_input
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev, check)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift,
                    x_stride=xb.stride(0) if nb > 1 else 0)
    if hold is not None:
        return _hold_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend else 0, xb, nb, n_fft // 2 + 1, scale, hold, workspace,
                          dev, table, x.dim() == 1, family, bool(onesided_doubling))
    return _welch_fft_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend else 0, xb, nb, n_fft // 2 + 1, scale,
                           onesided_doubling, out, workspace, dev, table, x.dim() == 1, family)


def welch_fft(params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
              onesided_doubling=True, shift=None, out=None, workspace=None):
    """The averaged periodogram of the rows of stft() WITHOUT the spectrum ever reaching memory (bhw_welch_fft_f32_device): x (T,) or
    (B, T), real float32, framed, windowed and transformed exactly as stft(params, x, n_fft, hop, win_length=..., center=...,
    pad_mode=..., detrend=...) does -- the (re, im) of every bin are the same words -- and |Y|^2 summed over the frames in the same
    kernel.  Returns float32 (K,) or (B, K), K = n_fft // 2 + 1: P[b, k] = fl32(A * scale * (2 for the doubled bins under
    onesided_doubling: every bin but 0 and n_fft / 2)), A the binary64 sum of re^2 + im^2 in the fixed order of include/bhw.h:
    ascending frames inside chunks of 16, the chunks of a block of 256 frames in order, then the blocks in order.  So P does not
    depend on B or the plan; for F <= 16 frames it is welch_psd(stft(...), scale, nfft=n_fft) bit for bit, for more frames within one
    float32 ulp of it.  center=True averages a centred (reflect- or zero-padded) spectrogram over time.  n_fft: a power of two in
    16..4096 (ValueError otherwise; complex x too).  `out`: float32 of the returned shape, bins contiguous, rows apart (its gaps are
    left alone); `workspace`: float64, B.welch_fft_workspace_bytes(...) // 8 elements (allocated when not given).  With both given
    the call neither allocates nor synchronises and can be captured with no warm call."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift, out,
                          workspace, x.device.index, None)


def _welch_fused(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace, dev, table, cache, family="fft",
                 hold=None):
    """hold: None (the mean: welch_fused*), or (traces, out_max, out_min) for hold_fused*: the same checks, window sums and
    frequency axis (the same cache keys), the scale of ONE frame's periodogram, and _hold_call in place of _welch_fft_call."""
    if hold is not None:
        B.hold_traces(hold[0])
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    L = int(length)
    noverlap = L // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < L:
        raise ValueError("noverlap must be less than length")
    nfft = L if nfft is None else int(nfft)
    hop = L - noverlap
    if hold is not None:
        (_hold_fft_input if family == "fft" else _hold_mfft_input)(torch, x, nfft, dev)
    else:
        (_fft_input if family == "fft" else _welch_mfft_input)(torch, x, nfft, dev)
    if not 1 <= L <= 1 << params.phi_width:
        raise ValueError(f"length {L} outside 1..2^phi_width = {1 << params.phi_width}")
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    if nb < 1 or T < L:
        raise ValueError(f"zero segments: T = {T} < length = {L}" if nb else "zero signals")
    frames = 1 + (T - L) // hop
    xb = _stft_input(xb, (T,))
    sums = _window_sums(torch, params, L, True, shift, dev, table, cache)
    scale = B.welch_scale(sums, frames if hold is None else 1, fs, scaling)
    sh = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, hop, nfft, shift=sh, x_stride=xb.stride(0) if nb > 1 else 0)
    # before the launch: it refuses inside a capture when missing
    freqs = _freq_axis(torch, cache, nfft, fs, dev, "freqs" if family == "fft" else "freqs_mixed")
    if hold is not None:
        return (freqs,) + _hold_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0, xb, nb,
                                     nfft // 2 + 1, scale, hold, workspace, dev, table, x.dim() == 1, family, True)
    P = _welch_fft_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0, xb, nb, nfft // 2 + 1, scale,
                        True, out, workspace, dev, table, x.dim() == 1, family)
    return freqs, P


_FREQS_KEPT = 8         # frequency axes a sums cache keeps (the oldest goes first)


def _freq_axis(torch, cache, nfft, fs, dev, kind="freqs"):
    """The float64 frequency axis welch_fused returns, built once per (nfft, fs) and kept beside the window sums in `cache` (the
    library's, or the table's own), so that a warm call allocates nothing.  Like the sums it is never made inside a capture: a tensor
    allocated there belongs to the graph's pool and holds nothing until the graph is replayed.  kind: the first word of the key,
    "freqs" for welch_fused and "freqs_mixed" for welch_fused_mixed, so that neither meets the other's axes or counts against them."""
    key = (kind, int(nfft), float(fs), int(dev))
    hit = cache.get(key)
    if hit is not None:
        return hit
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the frequency axis of this (nfft, fs) has not been built yet: call once outside the capture")
    kept = [k for k in cache if isinstance(k, tuple) and k and k[0] == kind]
    for k in kept[:max(0, len(kept) - _FREQS_KEPT + 1)]:
        del cache[k]
    axis = cache[key] = torch.fft.rfftfreq(int(nfft), d=1.0 / float(fs), dtype=torch.float64, device=f"cuda:{dev}")
    return axis


def welch_fused(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None, out=None,
                workspace=None):
    """welch(..., fft="fused") in ONE kernel and a small join (bhw_welch_fft_f32_device): the segments, their FFT and the average
    over them come from the same kernel, so the (B, F, K) spectrum that route writes and reads back never exists.  The arguments,
    their checks, the window sums (read once per (params, length, shift) and cached) and the scale are welch()'s for fft="fused";
    the result is the one-sided estimate (freqs float64, Pxx float32 (..., K)) -- the two-sided one is welch(return_onesided=False),
    and only the mean is averaged.  The sum over the frames has the order of welch_fft(), so Pxx equals welch(fft="fused") bit for
    bit up to 16 segments and within one float32 ulp beyond.  After one warm call, with `out` and `workspace` given, it neither
    synchronises nor allocates and can be captured (ResidentTable.welch_fused); a first call inside a capture -- the first for its
    window sums, or for its (nfft, fs) -- raises, as welch does.  `freqs` is SHARED and read-only: the same tensor is returned to
    every call with that (nfft, fs) (welch builds a new one each time), so copy it before changing it in place."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fused(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace, x.device.index, None,
                        _SUMS_CACHE)


# ---- fused Welch PSD at a mixed-radix n_fft: window, mixed-radix FFT and the frame average in one kernel -----------------------------------

def _welch_mfft_input(torch, x, n_fft, dev):
    """_mfft_input for the fused Welch calls: the refusals name the Welch call that takes what this one does not."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a float32 CUDA tensor on the call's device")
    if x.dtype != torch.float32:
        raise ValueError(f"the mixed-radix fused Welch PSD takes real float32 input, got {x.dtype} (complex64 I/Q input at a "
                         "power-of-two n_fft: welch_fft_iq / welch_fused_iq)")
    if x.dim() not in (1, 2):
        raise ValueError("x must be (T,) or (B, T)")
    n = int(n_fft)
    if n > 0 and n & (n - 1) == 0:
        raise ValueError(f"n_fft {n} is a power of two: welch_fft / welch_fused transform it (one transform per n_fft)")
    if not B.mfft_supported(n):
        raise ValueError(f"the mixed-radix fused FFT takes n_fft even 2^a·3^b·5^c in {B.MFFT_MIN_N}..{B.MFFT_MAX_N}, got {n}")


def welch_fft_mixed(params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                    onesided_doubling=True, shift=None, out=None, workspace=None):
    """welch_fft() at the n_fft of stft_mixed() (bhw_welch_mfft_f32_device): even, 2^a·3^b·5^c, in 16..4095 and not a power of two
    -- 400, 480, 960, 1000, 4000, the lengths that make the bin spacing a round number of hertz.  x (T,) or (B, T), real float32,
    framed, windowed and transformed exactly as stft_mixed(params, x, n_fft, hop, win_length=..., center=..., pad_mode=...,
    detrend=...) does -- the (re, im) of every bin are the same words -- and |Y|^2 summed over the frames in the same kernel, so the
    (B, F, K) spectrum never reaches memory.  Returns float32 (K,) or (B, K), K = n_fft // 2 + 1, with welch_fft()'s scale, doubling
    rule and order of the sums (chunks of 16 frames, blocks of 256, the blocks): P does not depend on B or the plan; for F <= 16
    frames it is welch_psd(stft_mixed(...), scale, nfft=n_fft) bit for bit, for more frames within one float32 ulp of it.  A
    power-of-two n_fft raises ValueError (welch_fft transforms it), complex x too (welch_fft_iq).  `out` and `workspace`
    (B.welch_mfft_workspace_bytes(...) // 8 float64 elements) as welch_fft(): with both given the call neither allocates nor
    synchronises and can be captured with no warm call."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift, out,
                          workspace, x.device.index, None, "mfft")


def welch_fused_mixed(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                      out=None, workspace=None):
    """welch_fused() at a mixed-radix nfft (bhw_welch_mfft_f32_device): scipy.signal.welch's segments, their FFT at nfft = 400, 1000,
    4000 ... unpadded, and the average over them in ONE kernel and a small join.  The arguments, their checks, the window sums
    cache, the scale and the SHARED read-only `freqs` are welch_fused()'s (the axes are kept under keys of their own kind, so neither
    call evicts the other's); the result is the one-sided estimate (freqs float64, Pxx float32 (..., K)).  The sum over the frames
    has the order of welch_fft_mixed().  A power-of-two nfft raises ValueError (welch_fused), complex x too (welch_fused_iq).  After
    one warm call, with `out` and `workspace` given, it neither synchronises nor allocates and can be captured
    (ResidentTable.welch_fused_mixed); a first call inside a capture raises."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fused(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace, x.device.index, None,
                        _SUMS_CACHE, "mfft")


# ---- fused Welch PSD for I/Q input: window, complex FFT and the frame average in one kernel ------------------------------------------------

def _welch_cfft_call(torch, params, L, s, flags, xb, nb, n_fft, scale, out, workspace, dev, table, one_d, family="cfft"):
    """The output and workspace rules of the fused Welch PSD for I/Q input and its launch: P float32 (n_fft,) or (B, n_fft).
    family: "cfft" (a power-of-two n_fft) or "cmfft" (a mixed-radix one): the two calls take the same arguments."""
    lib = B.lib()
    if family == "cfft":
        ws_bytes, device_call, table_call = B.welch_cfft_workspace_bytes, lib.bhw_welch_cfft_f32_device, lib.bhw_welch_cfft_f32_from_table
    else:
        ws_bytes, device_call, table_call = B.welch_cmfft_workspace_bytes, lib.bhw_welch_cmfft_f32_device, lib.bhw_welch_cmfft_f32_from_table
    shape = (n_fft,) if one_d else (nb, n_fft)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=xb.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != xb.device or tuple(out.shape) != shape \
            or out.stride(-1) != 1 or (out.dim() == 2 and nb > 1 and out.stride(0) < n_fft):
        raise ValueError(f"out must be a float32 tensor of shape {shape} on x's device, contiguous along the bins, rows apart")
    need = ws_bytes(s) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=xb.device)
    else:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    tail = (ctypes.byref(s), flags, float(scale), ctypes.c_void_p(xb.data_ptr()), ctypes.c_void_p(out.data_ptr()),
            out.stride(0) if (out.dim() == 2 and nb > 1) else 0, ctypes.c_void_p(workspace.data_ptr()), workspace.numel() * 8)
    if table is None:
        B.check(device_call(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(table_call(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return out


def _welch_cfft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, out, workspace, dev,
                    table, family="cfft", hold=None):
    """hold: None (the mean: welch_fft_iq*), or (traces, out_max, out_min) for the max-hold / min-hold traces of the same call
    (hold_fft_iq*): the same checks of the input, the same descriptor and flags, _hold_call in place of _welch_cfft_call."""
    if hold is not None:
        B.hold_traces(hold[0])
    check = _cfft_input if family == "cfft" else _welch_cmfft_input
    n_fft, L, xb, nb, T, frames, d = _stft_front(torch, params, x, n_fft, hop, win_length, center, pad_mode, detrend, dev, check)
    if not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a complex64 CUDA tensor on the call's device")
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], channels=2, shift=shift,
                    x_stride=xb.stride(0) * 2 if nb > 1 else 0)
    flags = (B.WELCH_DETREND_CONSTANT if detrend else 0) | (B.CFFT_SHIFT if fftshift else 0)
    if hold is not None:
        return _hold_call(torch, params, L, s, flags, xb, nb, n_fft, scale, hold, workspace, dev, table, x.dim() == 1, family)
    return _welch_cfft_call(torch, params, L, s, flags, xb, nb, n_fft, scale, out, workspace, dev, table, x.dim() == 1, family)


def welch_fft_iq(params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False, shift=None,
                 fftshift=False, out=None, workspace=None):
    """The two-sided averaged periodogram of the rows of stft_iq() WITHOUT the spectrum ever reaching memory
    (bhw_welch_cfft_f32_device): x (T,) or (B, T), complex64, framed, windowed and transformed exactly as stft_iq(params, x, n_fft,
    hop, win_length=..., center=..., pad_mode=..., detrend=...) does -- the (re, im) of every bin are the same words -- and |Y|^2
    summed over the frames in the same kernel.  Returns float32 (n_fft,) or (B, n_fft): P[b, j] = fl32(A * scale), A the binary64
    sum of re^2 + im^2 in the fixed order of include/bhw.h (welch_fft's: ascending frames inside chunks of 16, the chunks of a block
    of 256 frames in order, then the blocks in order); nothing is doubled.  So P does not depend on B or the plan; for F <= 16 frames
    it is welch_psd(stft_iq(...), scale, nfft=n_fft, onesided=False) bit for bit, for more frames within one float32 ulp of it.
    fftshift=True writes bin (j + n_fft // 2) % n_fft to column j: torch.fft.fftshift of the same values.  n_fft: a power of two in
    16..2048 (ValueError otherwise; a real or complex128 x too: welch_fft() takes real input).  `out`: float32 of the returned shape,
    bins contiguous, rows apart (its gaps are left alone); `workspace`: float64, B.welch_cfft_workspace_bytes(...) // 8 elements
    (allocated when not given).  With both given the call neither allocates nor synchronises and can be captured with no warm
    call."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_cfft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, out, workspace,
                           dev, None)


def _freq_axis_iq(torch, cache, nfft, fs, fftshift, dev, kind="freqs_iq"):
    """_freq_axis for welch_fused_iq: the two-sided axis fftfreq(nfft, 1 / fs), or its fftshift, kept beside the window sums under a
    key of its own kind ("freqs_iq"; welch_fused_iq_mixed: "freqs_iq_mixed"), so that it never meets welch_fused's one-sided axes,
    the other I/Q call's axes, or their counts."""
    key = (kind, int(nfft), float(fs), int(dev), bool(fftshift))
    hit = cache.get(key)
    if hit is not None:
        return hit
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the frequency axis of this (nfft, fs) has not been built yet: call once outside the capture")
    kept = [k for k in cache if isinstance(k, tuple) and k and k[0] == kind]
    for k in kept[:max(0, len(kept) - _FREQS_KEPT + 1)]:
        del cache[k]
    axis = torch.fft.fftfreq(int(nfft), d=1.0 / float(fs), dtype=torch.float64, device=f"cuda:{dev}")
    cache[key] = torch.fft.fftshift(axis) if fftshift else axis
    return cache[key]


def _welch_fused_iq(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, out, workspace, dev, table, cache,
                    family="cfft", hold=None):
    """hold: None (the mean: welch_fused_iq*), or (traces, out_max, out_min) for hold_fused_iq*: the same checks, window sums and
    frequency axis (the same cache keys), the scale of ONE frame's periodogram, and _hold_call in place of _welch_cfft_call."""
    if hold is not None:
        B.hold_traces(hold[0])
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    L = int(length)
    noverlap = L // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < L:
        raise ValueError("noverlap must be less than length")
    nfft = L if nfft is None else int(nfft)
    hop = L - noverlap
    (_cfft_input if family == "cfft" else _welch_cmfft_input)(torch, x, nfft, dev)
    if not x.is_cuda or x.device.index != dev:
        raise ValueError("x must be a complex64 CUDA tensor on the call's device")
    if not 1 <= L <= 1 << params.phi_width:
        raise ValueError(f"length {L} outside 1..2^phi_width = {1 << params.phi_width}")
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    xb = x if x.dim() == 2 else x.unsqueeze(0)
    nb, T = xb.shape
    if nb < 1 or T < L:
        raise ValueError(f"zero segments: T = {T} < length = {L}" if nb else "zero signals")
    frames = 1 + (T - L) // hop
    xb = _stft_input(xb, (T,))
    sums = _window_sums(torch, params, L, True, shift, dev, table, cache)
    scale = B.welch_scale(sums, frames if hold is None else 1, fs, scaling)
    sh = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, hop, nfft, channels=2, shift=sh, x_stride=xb.stride(0) * 2 if nb > 1 else 0)
    # before the launch: it refuses inside a capture when missing
    freqs = _freq_axis_iq(torch, cache, nfft, fs, fftshift, dev, "freqs_iq" if family == "cfft" else "freqs_iq_mixed")
    flags = (B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0) | (B.CFFT_SHIFT if fftshift else 0)
    if hold is not None:
        return (freqs,) + _hold_call(torch, params, L, s, flags, xb, nb, nfft, scale, hold, workspace, dev, table, x.dim() == 1, family)
    P = _welch_cfft_call(torch, params, L, s, flags, xb, nb, nfft, scale, out, workspace, dev, table, x.dim() == 1, family)
    return freqs, P


def welch_fused_iq(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                   fftshift=False, out=None, workspace=None):
    """welch() of a complex64 (I/Q) x in ONE kernel and a small join (bhw_welch_cfft_f32_device): the segments, their complex FFT and
    the average over them come from the same kernel, so the (B, F, nfft) spectrum never exists.  The arguments, their checks, the
    window sums (read once per (params, length, shift) and cached) and the scale are welch()'s for complex input; the result is the
    two-sided estimate (freqs float64, Pxx float32 (..., nfft)), freqs = fftfreq(nfft, 1 / fs), or with fftshift=True both freqs and
    Pxx in ascending frequency (torch.fft.fftshift of the same values).  Only the mean is averaged.  nfft: a power of two in 16..2048
    (ValueError otherwise; a real or complex128 x too).  The sum over the frames has the order of welch_fft_iq().  After one warm
    call, with `out` and `workspace` given, it neither synchronises nor allocates and can be captured
    (ResidentTable.welch_fused_iq); a first call inside a capture -- the first for its window sums, or for its (nfft, fs, fftshift)
    -- raises, as welch_fused does.  `freqs` is SHARED and read-only, as welch_fused's."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_fused_iq(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, out, workspace, dev, None,
                           _SUMS_CACHE)


# ---- fused Welch PSD for I/Q input at a mixed-radix n_fft: window, mixed-radix complex FFT and the frame average in one kernel ------------

def _welch_cmfft_input(torch, x, n_fft, dev):
    """_cmfft_input for the fused Welch calls: the refusals name the Welch call that takes what this one does not."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.complex64:
        got = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"the mixed-radix fused Welch PSD for I/Q input takes complex64 input, got {got} (real input at a "
                         "mixed-radix n_fft: welch_fft_mixed / welch_fused_mixed)")
    n = int(n_fft)
    if x.dim() in (1, 2) and n > 0 and n & (n - 1) == 0:
        raise ValueError(f"n_fft {n} is a power of two: welch_fft_iq / welch_fused_iq transform it (one transform per n_fft)")
    _cmfft_input(torch, x, n_fft, dev)


def welch_fft_iq_mixed(params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False, shift=None,
                       fftshift=False, out=None, workspace=None):
    """welch_fft_iq() at the n_fft of stft_iq_mixed() (bhw_welch_cmfft_f32_device): 2^a·3^b·5^c in 16..2047 that is no power of two,
    odd lengths included -- 400, 1000, 1200, 1536, 2000, 2025.  x (T,) or (B, T), complex64, framed, windowed and transformed exactly
    as stft_iq_mixed(params, x, n_fft, hop, win_length=..., center=..., pad_mode=..., detrend=...) does -- the (re, im) of every bin
    are the same words -- and |Y|^2 summed over the frames in the same kernel, so the (B, F, n_fft) spectrum never reaches memory.
    Returns float32 (n_fft,) or (B, n_fft) with welch_fft_iq()'s scale and order of the sums (chunks of 16 frames, blocks of 256, the
    blocks); nothing is doubled.  P does not depend on B or the plan; for F <= 16 frames it is welch_psd(stft_iq_mixed(...), scale,
    nfft=n_fft, onesided=False) bit for bit, for more frames within one float32 ulp of it.  fftshift=True writes bin
    (j + n_fft - n_fft // 2) % n_fft to column j: torch.fft.fftshift of the same values, for an odd n_fft too.  A power-of-two n_fft
    raises ValueError (welch_fft_iq transforms it), real x too (welch_fft_mixed), complex128 and every other n_fft too.  `out` and
    `workspace` (B.welch_cmfft_workspace_bytes(...) // 8 float64 elements) as welch_fft_iq(): with both given the call neither
    allocates nor synchronises and can be captured with no warm call."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_cfft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, out, workspace,
                           dev, None, "cmfft")


def welch_fused_iq_mixed(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                         fftshift=False, out=None, workspace=None):
    """welch_fused_iq() at a mixed-radix nfft (bhw_welch_cmfft_f32_device): scipy.signal.welch's segments of a complex64 x, their
    complex FFT at nfft = 400, 1000, 1536, 2025 ... unpadded, and the average over them in ONE kernel and a small join.  The
    arguments, their checks, the window sums cache and the scale are welch_fused_iq()'s; the result is the two-sided estimate (freqs
    float64, Pxx float32 (..., nfft)), freqs = fftfreq(nfft, 1 / fs), or with fftshift=True both freqs and Pxx in ascending frequency
    (torch.fft.fftshift of the same values).  The SHARED read-only `freqs` are kept under keys of their own kind, so neither I/Q call
    evicts the other's.  Only the mean is averaged.  The sum over the frames has the order of welch_fft_iq_mixed().  A power-of-two
    nfft raises ValueError (welch_fused_iq), real x too (welch_fused_mixed).  After one warm call, with `out` and `workspace` given,
    it neither synchronises nor allocates and can be captured (ResidentTable.welch_fused_iq_mixed); a first call inside a capture
    raises."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_fused_iq(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, out, workspace, dev, None,
                           _SUMS_CACHE, "cmfft")


# ---- fused max-hold / min-hold traces for I/Q input: window, complex FFT and the extrema over the frames in one kernel -------------------

def _hold_call(torch, params, L, s, flags, xb, nb, n_fft, scale, hold, workspace, dev, table, one_d, family, onesided=None):
    """The output and workspace rules of the fused hold calls and their launch: (pmax, pmin), each float32 (n_fft,) or (B, n_fft)
    or None for the trace not asked for.  The rules of each output are those of welch_fft_iq's `out`; both given share one row
    stride (the C call has one p_stride).  For the real-input families "fft" and "mfft" n_fft counts the K columns of a row and
    `onesided` is the doubling the C call takes as psd_flags behind the scale; the I/Q families have no such argument."""
    traces, out_max, out_min = hold
    mask = B.hold_traces(traces)
    lib = B.lib()
    if family == "cfft":
        ws_bytes, device_call, table_call = B.hold_cfft_workspace_bytes, lib.bhw_hold_cfft_f32_device, lib.bhw_hold_cfft_f32_from_table
    elif family == "cmfft":
        ws_bytes, device_call, table_call = B.hold_cmfft_workspace_bytes, lib.bhw_hold_cmfft_f32_device, lib.bhw_hold_cmfft_f32_from_table
    elif family == "fft":
        ws_bytes, device_call, table_call = B.hold_fft_workspace_bytes, lib.bhw_hold_fft_f32_device, lib.bhw_hold_fft_f32_from_table
    else:
        ws_bytes, device_call, table_call = B.hold_mfft_workspace_bytes, lib.bhw_hold_mfft_f32_device, lib.bhw_hold_mfft_f32_from_table
    shape = (n_fft,) if one_d else (nb, n_fft)
    outs = []
    for bit, name, out in ((B.HOLD_MAX, "out_max", out_max), (B.HOLD_MIN, "out_min", out_min)):
        if not mask & bit:
            if out is not None:
                raise ValueError(f"{name} is given but traces={traces!r} does not ask for that trace")
        elif out is None:
            out = torch.empty(shape, dtype=torch.float32, device=xb.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != xb.device or tuple(out.shape) != shape \
                or out.stride(-1) != 1 or (out.dim() == 2 and nb > 1 and out.stride(0) < n_fft):
            raise ValueError(f"{name} must be a float32 tensor of shape {shape} on x's device, contiguous along the bins, rows apart")
        outs.append(out)
    pmax, pmin = outs
    strides = {o.stride(0) for o in outs if o is not None and o.dim() == 2 and nb > 1}
    if len(strides) > 1:
        raise ValueError("out_max and out_min must have the same row stride")
    need = ws_bytes(s) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=xb.device)
    else:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    ptr = lambda o: ctypes.c_void_p(o.data_ptr()) if o is not None else None   # noqa: E731
    psd = () if onesided is None else (B.PSD_ONESIDED if onesided else 0,)
    tail = (ctypes.byref(s), flags, float(scale)) + psd + (ctypes.c_void_p(xb.data_ptr()), ptr(pmax), ptr(pmin),
            strides.pop() if strides else 0, ctypes.c_void_p(workspace.data_ptr()), workspace.numel() * 8)
    if table is None:
        B.check(device_call(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(table_call(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return pmax, pmin


def hold_fft_iq(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False, shift=None,
                fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
    """The max-hold and min-hold traces of the rows of spectrogram_iq() WITHOUT the powers ever reaching memory
    (bhw_hold_cfft_f32_device): x (T,) or (B, T), complex64, framed, windowed and transformed exactly as spectrogram_iq(params, x,
    n_fft, hop, win_length=..., center=..., pad_mode=..., detrend=..., fftshift=...) does -- the float32 power of every bin is the
    same word -- and reduced over the frames in the same kernel.  Returns (pmax, pmin), each float32 (n_fft,) or (B, n_fft):
    pmax = (S.amax(-2).double() * scale).float() and pmin the same with amin, S that spectrogram, BIT FOR BIT at every number of
    frames (a maximum has no order of summation), a NaN in any frame of a bin making both traces of it NaN as amax / amin do.  So
    the traces do not depend on B or the plan.  traces: "both" | "max" | "min"; the trace not asked for is None and is not
    written.  n_fft: a power of two in 16..2048; the arguments, their checks and ValueErrors are welch_fft_iq()'s.  `out_max`,
    `out_min`: float32 of the returned shape, bins contiguous, rows apart by the same stride (gaps are left alone); `workspace`:
    float64, B.hold_cfft_workspace_bytes(...) // 8 elements (allocated when not given).  With the outputs and the workspace given
    the call neither allocates nor synchronises and can be captured with no warm call.  The mean of the same frames is
    welch_fft_iq(); a median is not built."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_cfft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, None, workspace,
                           dev, None, "cfft", (traces, out_max, out_min))


def hold_fft_iq_mixed(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False, shift=None,
                      fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
    """hold_fft_iq() at the n_fft of stft_iq_mixed() (bhw_hold_cmfft_f32_device): 2^a·3^b·5^c in 16..2047 that is no power of two,
    odd lengths included.  The traces are those of spectrogram_iq_mixed()'s rows, bit for bit; with fftshift=True an odd n_fft follows
    torch.fft.fftshift.  The arguments, their checks and ValueErrors are welch_fft_iq_mixed()'s: a power-of-two n_fft raises
    (hold_fft_iq transforms it), real x too.  `workspace`: B.hold_cmfft_workspace_bytes(...) // 8 float64 elements."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_cfft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, None, workspace,
                           dev, None, "cmfft", (traces, out_max, out_min))


def hold_fused_iq(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                  fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
    """The max-hold and min-hold traces beside welch_fused_iq()'s mean (bhw_hold_cfft_f32_device): scipy.signal.welch's segments of
    a complex64 x, their complex FFT, and the largest and the smallest periodogram value of every bin over the segments, in ONE
    kernel and a small join.  The arguments, their checks, the window sums cache and the SHARED read-only `freqs` are
    welch_fused_iq()'s (the same tensors under the same keys); the scale is that of ONE segment's periodogram, so the traces are in
    the units of welch_fused_iq()'s Pxx and bracket it.  Returns (freqs, pmax, pmin); traces, out_max, out_min and workspace as
    hold_fft_iq(), whose traces at that scale these are bit for bit.  After one warm call it can be captured
    (ResidentTable.hold_fused_iq); a first call inside a capture raises, as welch_fused_iq does."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_fused_iq(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, None, workspace, dev, None,
                           _SUMS_CACHE, "cfft", (traces, out_max, out_min))


def hold_fused_iq_mixed(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                        fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
    """hold_fused_iq() at a mixed-radix nfft (bhw_hold_cmfft_f32_device): the checks, the caches and `freqs` are
    welch_fused_iq_mixed()'s."""
    torch = _torch()
    dev = x.device.index if isinstance(x, torch.Tensor) and x.is_cuda else None
    return _welch_fused_iq(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, None, workspace, dev, None,
                           _SUMS_CACHE, "cmfft", (traces, out_max, out_min))


# ---- fused max-hold / min-hold traces for real input: window, real FFT and the extrema over the frames in one kernel -----------------------

def _hold_fft_input(torch, x, n_fft, dev):
    """_fft_input for hold_fft / hold_fused: what this call does not take is refused in the name of the hold call that does."""
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"the fused hold traces for real input take real float32 input, got {x.dtype} (complex64 I/Q input: "
                         "hold_fft_iq / hold_fused_iq)")
    if B.mfft_supported(n_fft):
        raise ValueError(f"n_fft {int(n_fft)} is mixed-radix: hold_fft_mixed / hold_fused_mixed transform it (one transform per n_fft)")
    _fft_input(torch, x, n_fft, dev)


def _hold_mfft_input(torch, x, n_fft, dev):
    """_welch_mfft_input for hold_fft_mixed / hold_fused_mixed, with the refusals in the hold calls' names."""
    if isinstance(x, torch.Tensor) and x.is_complex():
        raise ValueError(f"the mixed-radix fused hold traces for real input take real float32 input, got {x.dtype} (complex64 I/Q "
                         "input: hold_fft_iq_mixed / hold_fused_iq_mixed)")
    n = int(n_fft)
    if n > 0 and n & (n - 1) == 0:
        raise ValueError(f"n_fft {n} is a power of two: hold_fft / hold_fused transform it (one transform per n_fft)")
    _welch_mfft_input(torch, x, n_fft, dev)


def hold_fft(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
             onesided_doubling=True, shift=None, traces="both", out_max=None, out_min=None, workspace=None):
    """The max-hold and min-hold traces of the rows of spectrogram() WITHOUT the powers ever reaching memory
    (bhw_hold_fft_f32_device): x (T,) or (B, T), real float32, framed, windowed and transformed exactly as spectrogram(params, x,
    n_fft, hop, win_length=..., center=..., pad_mode=..., detrend=...) does -- the float32 power of every bin is the same word -- and
    reduced over the frames in the same kernel.  Returns (pmax, pmin), each float32 (K,) or (B, K), K = n_fft // 2 + 1:
    pmax = (S.amax(-2).double() * sk).float() and pmin the same with amin, S that spectrogram and sk = scale * (2 for the doubled
    bins under onesided_doubling: every bin but 0 and n_fft / 2), welch_fft()'s factor, BIT FOR BIT at every number of frames (a
    maximum has no order of summation); a NaN in any frame of a bin makes both traces of it NaN as amax / amin do.  So the traces do
    not depend on B or the plan.  traces: "both" | "max" | "min"; the trace not asked for is None and is not written.  n_fft: a power
    of two in 16..4096; the arguments and their checks are welch_fft()'s, a mixed-radix n_fft raises ValueError (hold_fft_mixed
    transforms it), complex x too (hold_fft_iq).  `out_max`, `out_min`: float32 of the returned shape, bins contiguous, rows apart by
    the same stride (gaps are left alone); `workspace`: float64, B.hold_fft_workspace_bytes(...) // 8 elements (allocated when not
    given).  With the outputs and the workspace given the call neither allocates nor synchronises and can be captured with no warm
    call.  The mean of the same frames is welch_fft(); a median is not built."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift, None,
                          workspace, x.device.index, None, "fft", (traces, out_max, out_min))


def hold_fft_mixed(params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                   onesided_doubling=True, shift=None, traces="both", out_max=None, out_min=None, workspace=None):
    """hold_fft() at the n_fft of stft_mixed() (bhw_hold_mfft_f32_device): even, 2^a·3^b·5^c, in 16..4095 and not a power of two --
    400, 480, 960, 1000, 4000.  The traces are those of spectrogram_mixed()'s rows, bit for bit.  The arguments and their checks are
    welch_fft_mixed()'s: a power-of-two n_fft raises ValueError (hold_fft transforms it), complex x too (hold_fft_iq_mixed).
    `workspace`: B.hold_mfft_workspace_bytes(...) // 8 float64 elements."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fft_psd(torch, params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift, None,
                          workspace, x.device.index, None, "mfft", (traces, out_max, out_min))


def hold_fused(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
               traces="both", out_max=None, out_min=None, workspace=None):
    """The max-hold and min-hold traces beside welch_fused()'s mean (bhw_hold_fft_f32_device): scipy.signal.welch's segments, their
    FFT, and the largest and the smallest periodogram value of every bin over the segments, in ONE kernel and a small join.  The
    arguments, their checks, the window sums cache and the SHARED read-only `freqs` are welch_fused()'s (the same tensors under the
    same keys); the scale is that of ONE segment's periodogram, so the traces are in the units of welch_fused()'s Pxx and bracket
    it: pmin <= Pxx <= pmax.  Returns (freqs, pmax, pmin); traces, out_max, out_min and workspace as hold_fft(), whose traces at that
    scale these are bit for bit.  After one warm call it can be captured (ResidentTable.hold_fused); a first call inside a capture
    raises, as welch_fused does."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fused(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, None, workspace, x.device.index, None,
                        _SUMS_CACHE, "fft", (traces, out_max, out_min))


def hold_fused_mixed(params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                     traces="both", out_max=None, out_min=None, workspace=None):
    """hold_fused() at a mixed-radix nfft (bhw_hold_mfft_f32_device): the checks, the caches and `freqs` are welch_fused_mixed()'s."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a float32 CUDA tensor")
    return _welch_fused(torch, params, x, fs, length, noverlap, nfft, detrend, scaling, shift, None, workspace, x.device.index, None,
                        _SUMS_CACHE, "mfft", (traces, out_max, out_min))


# ---- Welch cross spectra: the pass behind the FFT for two signals -------------------------------------------------------------------------

def _csd_operand(torch, t, what, dev):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.complex64 or t.device.index != dev:
        raise ValueError(f"{what} must be a complex64 CUDA tensor on the call's device")
    if t.dim() not in (2, 3):
        raise ValueError(f"{what} must be (frames, bins) or (B, frames, bins)")
    tb = t if t.dim() == 3 else t.unsqueeze(0)
    nb, F, K = tb.shape
    if nb < 1 or F < 1 or K < 1:
        raise ValueError(f"{what} has no signals, frames or bins")
    return _stft_input(tb, ((F - 1) * max(tb.stride(1), K) + K, K))


def welch_csd(X, Y, scale, *, nfft, onesided=True, outputs=("pxy",), out=None, workspace=None):
    """Welch cross spectra behind the FFT (bhw_welch_csd_f32): X, Y complex64 (F, K) or (B, F, K), the FFTs of the segments of x and
    of y.  One pass reads X and Y once and returns a dict with the `outputs` asked for, each (K,) or (B, K) as Y is: "pxy" complex64,
    the averaged conj(X) * Y times scale (scipy.signal.csd's convention); "pxx", "pyy" float32, bit for bit welch_psd of X and of Y;
    "coherence" float32, |sum conj(X) Y|^2 / (sum |X|^2 * sum |Y|^2); "h1" complex64, the transfer-function estimate P_xy / P_xx.
    All come from the same four binary64 sums, in ascending f inside blocks of 256 frames and then over the blocks in order
    (include/bhw.h writes the arithmetic down).  X of one signal -- (F, K) or (1, F, K) -- against Y of B signals is paired with
    each of them.  onesided as welch_psd.  X and Y are read in place when their bins are contiguous and their rows apart, else
    copied.  `out`: a dict by output name of tensors of the returned shape and dtype, last axis contiguous, all with the same row
    stride (their gaps are left alone); `workspace`: float64, B * ceil(F / 256) * K * chains elements when F > 256 (chains = 2 for
    "pxy" alone, else 4; allocated when not given)."""
    torch = _torch()
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda:
        raise ValueError("Y must be a complex64 CUDA tensor on the call's device")
    dev = Y.device.index
    mask = B.csd_mask(outputs)
    names = [n for n in B.CSD_OUTPUTS if B.CSD_OUTPUTS[n][0] & mask]
    Xb, Yb = _csd_operand(torch, X, "X", dev), _csd_operand(torch, Y, "Y", dev)
    nb, F, K = Yb.shape
    if X.dim() == 3 and Y.dim() == 2:
        raise ValueError("a batched X (B, frames, bins) needs a batched Y")
    if tuple(Xb.shape[1:]) != (F, K) or Xb.shape[0] not in (1, nb):
        raise ValueError(f"X {tuple(X.shape)} and Y {tuple(Y.shape)} must have the same frames and bins, and X one signal or Y's {nb}")
    bcast = Xb.shape[0] == 1 and nb > 1
    nfft = int(nfft)
    if onesided and K != nfft // 2 + 1:
        raise ValueError(f"a one-sided spectrum of nfft {nfft} has {nfft // 2 + 1} bins, X and Y have {K}")
    if K > nfft:
        raise ValueError(f"X and Y have {K} bins, more than nfft {nfft}")
    shape = (nb, K) if Y.dim() == 3 else (K,)
    out = {} if out is None else out
    if not isinstance(out, dict) or any(n not in names for n in out):
        raise ValueError(f"out must be a dict of tensors by output name, within the outputs asked for {tuple(names)}")
    res, o_stride = {}, None
    for n in names:
        dt = torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32
        t = out.get(n)
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != Y.device or tuple(t.shape) != shape or t.is_conj() or t.is_neg() \
                or (K > 1 and t.stride(-1) != 1) or (t.dim() == 2 and nb > 1 and t.stride(0) < K):
            raise ValueError(f"out[{n!r}] must be a {str(dt).replace('torch.', '')} tensor of shape {shape} on Y's device, contiguous along "
                             "the bins, rows apart")
        if t.dim() == 2 and nb > 1:
            if o_stride not in (None, t.stride(0)):
                raise ValueError("the tensors of out must have the same row stride (bhw_csd.o_stride is one number)")
            o_stride = t.stride(0)
        res[n] = t
    for n in names:
        if n not in res:
            dt = torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32
            if o_stride in (None, K):
                res[n] = torch.empty(shape, dtype=dt, device=Y.device)
            else:
                res[n] = torch.empty((nb, o_stride), dtype=dt, device=Y.device)[:, :K]
    d = B.make_csd(nb, F, K, nfft, scale, outputs=names, onesided=onesided, broadcast_x=bcast,
                   x_stride=Xb.stride(1) if F > 1 else 0, x_batch_stride=Xb.stride(0) if (nb > 1 and not bcast) else 0,
                   y_stride=Yb.stride(1) if F > 1 else 0, y_batch_stride=Yb.stride(0) if nb > 1 else 0, o_stride=o_stride or 0)
    need = int(B.lib().bhw_welch_csd_workspace_bytes(ctypes.byref(d))) // 8
    if need and workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=Y.device)
    elif need:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    ptrs = [ctypes.c_void_p(res[n].data_ptr() if n in res else None) for n in B.CSD_OUTPUTS]
    B.check(B.lib().bhw_welch_csd_f32(dev, _stream_ptr(torch, dev), ctypes.byref(d), ctypes.c_void_p(Xb.data_ptr()),
                                      ctypes.c_void_p(Yb.data_ptr()), *ptrs, ctypes.c_void_p(workspace.data_ptr() if need else None),
                                      need * 8))
    return res


def _cross(torch, params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, outputs, table, cache, fft="torch"):
    """The chain of csd / coherence / transfer_function / cross_spectra: (freqs, dict by output name)."""
    fused = _fft_check(fft)
    for t, what in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what} must be a float32 or complex64 CUDA tensor")
    dev = x.device.index if table is None else table.device
    _stft_float(torch, x, "x", dev)
    _stft_float(torch, y, "y", dev)
    if x.dtype != y.dtype:
        raise ValueError(f"x and y must have the same dtype, got {x.dtype} and {y.dtype}")
    if x.dim() not in (1, 2) or y.dim() not in (1, 2):
        raise ValueError("x and y must be (T,) or (B, T)")
    if x.shape[-1] != y.shape[-1]:
        raise ValueError(f"x and y must have the same length, got {x.shape[-1]} and {y.shape[-1]} (scipy zero-pads the shorter one; "
                         "that is not built: pad or cut it yourself)")
    if x.dim() == 2 and (y.dim() == 1 or x.shape[0] != y.shape[0]):
        raise ValueError(f"x {tuple(x.shape)} against y {tuple(y.shape)}: x must be (T,) (paired with every signal of y) or have y's batch")
    B.csd_mask(outputs)
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    L, T = int(length), x.shape[-1]
    noverlap = L // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < L:
        raise ValueError("noverlap must be less than length")
    nfft = L if nfft is None else int(nfft)
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    if fused:                                                      # every refusal of the fused route before anything is launched or read
        if x.is_complex() or not return_onesided:
            raise ValueError("fft='fused' takes real x and y and gives the one-sided spectra only (otherwise: fft='torch')")
        _fft_input(torch, x, nfft, dev)
        _fft_input(torch, y, nfft, dev)
    if T < L or (y.dim() == 2 and y.shape[0] < 1):
        raise ValueError(f"zero segments: T = {T} < length = {L}" if T < L else "zero signals")
    hop = L - noverlap
    frames = 1 + (T - L) // hop
    sums = _window_sums(torch, params, L, True, shift, dev, None if table is None else table._live(), cache)
    scale = B.welch_scale(sums, frames, fs, scaling)
    # the segments of x and of y in one buffer, so that one FFT call transforms both
    nx = x.shape[0] if x.dim() == 2 else 1
    ny = y.shape[0] if y.dim() == 2 else 1
    if fused:
        # the spectra of x and of y by the fused kernel, two calls into the two halves of one buffer
        handle = None if table is None else table._live()
        S = torch.empty((nx + ny, frames, nfft // 2 + 1), dtype=torch.complex64, device=x.device)
        _welch_fft(torch, params, x, L, hop, nfft, detrend, shift, S[:nx] if x.dim() == 2 else S[0], dev, handle)
        _welch_fft(torch, params, y, L, hop, nfft, detrend, shift, S[nx:] if y.dim() == 2 else S[nx], dev, handle)
        res = welch_csd(S[:nx] if x.dim() == 2 else S[0], S[nx:] if y.dim() == 2 else S[nx], scale, nfft=nfft, onesided=True,
                        outputs=outputs)
        return torch.fft.rfftfreq(nfft, d=1.0 / float(fs), dtype=torch.float64, device=S.device), res
    seg = torch.empty((nx + ny, frames, nfft), dtype=x.dtype, device=x.device)
    handle = None if table is None else table._live()
    _welch_frames(torch, params, x, L, hop, nfft, detrend, shift, seg[:nx] if x.dim() == 2 else seg[0], None, dev, handle)
    _welch_frames(torch, params, y, L, hop, nfft, detrend, shift, seg[nx:] if y.dim() == 2 else seg[nx], None, dev, handle)
    onesided = bool(return_onesided) and not seg.is_complex()
    S = torch.fft.rfft(seg, dim=-1) if onesided else torch.fft.fft(seg, dim=-1)
    res = welch_csd(S[:nx] if x.dim() == 2 else S[0], S[nx:] if y.dim() == 2 else S[nx], scale, nfft=nfft, onesided=onesided,
                    outputs=outputs)
    mk = torch.fft.rfftfreq if onesided else torch.fft.fftfreq
    return mk(nfft, d=1.0 / float(fs), dtype=torch.float64, device=seg.device), res


def cross_spectra(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True, scaling="density",
                  shift=None, outputs=("pxy", "pxx", "pyy", "coherence", "h1"), fft="torch"):
    """Every Welch cross-spectral estimate of (x, y) from one pass, scipy.signal.csd / coherence as the model: x and y (T,) or (B, T)
    of the same length and dtype, float32 (one-sided, rfft) or complex64 (two-sided, fft); x (T,) against y (B, T) is paired with
    every signal of y.  Both are cut, detrended, windowed and zero-padded as welch() does, into ONE buffer that one torch.fft call
    transforms, and welch_csd reads the two spectra once: window_sums -> welch_frames(x), welch_frames(y) -> torch.fft -> welch_csd.
    Returns (freqs float64, dict by output name: "pxy" = scipy's csd(x, y), "pxx" / "pyy" = welch(x) / welch(y), "coherence" =
    scipy's coherence(x, y), "h1" = P_xy / P_xx).  The sums cache and the capture rule are welch()'s.  Signals of unequal length are a
    ValueError (scipy zero-pads the shorter one).  fft="fused": the segments and spectra of x and of y come from the fused window +
    FFT kernel (two calls into the two halves of one buffer; see welch() for what it takes and what it changes)."""
    return _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, outputs, None, _SUMS_CACHE,
                  fft)


def csd(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True, scaling="density",
        shift=None, fft="torch"):
    """Welch's cross power spectral density P_xy (scipy.signal.csd's convention, conj(X) * Y): cross_spectra() with outputs=("pxy",),
    the two-chain kernel.  Returns (freqs float64, Pxy complex64 (..., K))."""
    f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("pxy",), None, _SUMS_CACHE,
                  fft)
    return f, r["pxy"]


def coherence(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True, scaling="density",
              shift=None, fft="torch"):
    """The magnitude-squared coherence |P_xy|^2 / (P_xx P_yy) of scipy.signal.coherence, from one pass over both spectra.  Returns
    (freqs float64, Cxy float32 (..., K)); NaN in a bin where x or y has no power at all."""
    f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("coherence",), None,
                  _SUMS_CACHE, fft)
    return f, r["coherence"]


def transfer_function(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                      scaling="density", shift=None, fft="torch"):
    """The H1 estimate P_xy / P_xx of the transfer function from x (the excitation) to y (the response).  Returns (freqs float64,
    H1 complex64 (..., K))."""
    f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("h1",), None, _SUMS_CACHE,
                  fft)
    return f, r["h1"]


# ---- fused Welch cross spectra: window, FFT of x and of y and the four frame averages in one kernel ---------------------------------------

CSD_FFT_MAX_N = 2048


def _csd_fft_input(torch, x, y, n_fft, dev):
    """The checks of the fused cross spectra on (x, y, n_fft); the refusals name the route that takes what this one does not."""
    for t, what in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != dev:
            raise ValueError(f"{what} must be a float32 CUDA tensor on the call's device")
        if t.dtype != torch.float32:
            raise ValueError(f"the fused cross spectra take real float32 input, got {t.dtype} for {what} (complex input: "
                             "cross_spectra(fft='torch'), or stft_iq of x and of y + welch_csd)")
    if x.dim() not in (1, 2) or y.dim() not in (1, 2):
        raise ValueError("x and y must be (T,) or (B, T)")
    if x.shape[-1] != y.shape[-1]:
        raise ValueError(f"x and y must have the same length, got {x.shape[-1]} and {y.shape[-1]} (scipy zero-pads the shorter one; "
                         "that is not built: pad or cut it yourself)")
    if x.dim() == 2 and (y.dim() == 1 or x.shape[0] != y.shape[0]):
        raise ValueError(f"x {tuple(x.shape)} against y {tuple(y.shape)}: x must be (T,) (paired with every signal of y) or have y's batch")
    n = int(n_fft)
    if B.mfft_supported(n):
        raise ValueError(f"n_fft {n} is mixed-radix: the fused cross spectra take a power of two in {B.FFT_MIN_N}..{CSD_FFT_MAX_N} "
                         "(stft_mixed of x and of y + welch_csd take it)")
    if B.fft_supported(n) and n > CSD_FFT_MAX_N:
        raise ValueError(f"n_fft {n}: the fused cross spectra take a power of two in {B.FFT_MIN_N}..{CSD_FFT_MAX_N}, two operands side "
                         "by side (cross_spectra(fft='fused'), or stft of x and of y + welch_csd, take it)")
    if not B.fft_supported(n):
        raise ValueError(f"the fused cross spectra take n_fft a power of two in {B.FFT_MIN_N}..{CSD_FFT_MAX_N}, got {n}")


def _csd_fft_call(torch, params, L, s, flags, xb, yb, nb, K, scale, onesided, bcast, outputs, out, workspace, dev, table, one_d):
    """The output and workspace rules of the fused cross spectra (welch_csd's for `out`) and the launch: a dict by output name."""
    mask = B.csd_mask(outputs)
    names = [n for n in B.CSD_OUTPUTS if B.CSD_OUTPUTS[n][0] & mask]
    shape = (K,) if one_d else (nb, K)
    out = {} if out is None else out
    if not isinstance(out, dict) or any(n not in names for n in out):
        raise ValueError(f"out must be a dict of tensors by output name, within the outputs asked for {tuple(names)}")
    res, o_stride = {}, None
    for n in names:
        t = out.get(n)
        if t is None:
            continue
        dt = torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != yb.device or tuple(t.shape) != shape or t.is_conj() or t.is_neg() \
                or t.stride(-1) != 1 or (t.dim() == 2 and nb > 1 and t.stride(0) < K):
            raise ValueError(f"out[{n!r}] must be a {str(dt).replace('torch.', '')} tensor of shape {shape} on y's device, contiguous along "
                             "the bins, rows apart")
        if t.dim() == 2 and nb > 1:
            if o_stride not in (None, t.stride(0)):
                raise ValueError("the tensors of out must have the same row stride (o_stride is one number)")
            o_stride = t.stride(0)
        res[n] = t
    for n in names:
        if n not in res:
            dt = torch.complex64 if B.CSD_OUTPUTS[n][1] else torch.float32
            if o_stride in (None, K):
                res[n] = torch.empty(shape, dtype=dt, device=yb.device)
            else:
                res[n] = torch.empty((nb, o_stride), dtype=dt, device=yb.device)[:, :K]
    need = B.csd_fft_workspace_bytes(s) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=yb.device)
    else:
        _check_out(torch, workspace, need, "workspace", torch.float64)
    cflags = mask | (B.CSD_ONESIDED if onesided else 0) | (B.CSD_BROADCAST_X if bcast else 0)
    ptrs = [ctypes.c_void_p(res[n].data_ptr() if n in res else None) for n in B.CSD_OUTPUTS]
    tail = (ctypes.byref(s), flags, float(scale), cflags, ctypes.c_void_p(xb.data_ptr()), ctypes.c_void_p(yb.data_ptr()), *ptrs,
            o_stride or 0, ctypes.c_void_p(workspace.data_ptr()), workspace.numel() * 8)
    if table is None:
        B.check(B.lib().bhw_csd_fft_f32_device(ctypes.byref(params), L, dev, _stream_ptr(torch, dev), *tail))
    else:
        B.check(B.lib().bhw_csd_fft_f32_from_table(table, ctypes.byref(params), L, _stream_ptr(torch, dev), *tail))
    return res


def _csd_fft_operands(x, y):
    """(x read, y read, nb, bcast, batch stride) for x (T,) or (B, T) against y: one batch stride serves both operands."""
    yb = _stft_input(y if y.dim() == 2 else y.unsqueeze(0), (y.shape[-1],))
    xb = _stft_input(x if x.dim() == 2 else x.unsqueeze(0), (x.shape[-1],))
    nb, T = yb.shape
    bcast = xb.shape[0] == 1 and nb > 1
    if nb > 1 and not bcast and xb.stride(0) != yb.stride(0):           # one bhw_stft describes both: the same batch stride
        xb, yb = xb.contiguous(), yb.contiguous()
    return xb, yb, nb, bcast, (yb.stride(0) if nb > 1 else 0)


def _csd_fft(torch, params, x, y, n_fft, hop, scale, outputs, win_length, center, pad_mode, detrend, onesided_doubling, shift, out,
             workspace, dev, table):
    check = lambda torch, t, n, dev: _csd_fft_input(torch, x, y, n, dev)
    n_fft, L, _, _, T, frames, d = _stft_front(torch, params, y, n_fft, hop, win_length, center, pad_mode, detrend, dev, check)
    xb, yb, nb, bcast, bs = _csd_fft_operands(x, y)
    shift = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, d["hop"], n_fft, col0=d["col0"], pad=d["pad"], pad_mode=d["pad_mode"], shift=shift, x_stride=bs)
    return _csd_fft_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend else 0, xb, yb, nb, n_fft // 2 + 1, scale,
                         onesided_doubling, bcast, outputs, out, workspace, dev, table, y.dim() == 1)


def csd_fft(params, x, y, n_fft, hop, scale, *, outputs=("pxy",), win_length=None, center=False, pad_mode="reflect", detrend=False,
            onesided_doubling=True, shift=None, out=None, workspace=None):
    """welch_csd(stft(x), stft(y)) WITHOUT either spectrum ever reaching memory (bhw_csd_fft_f32_device): x and y real float32 of the
    same length, (T,) or (B, T) -- x (T,) against y (B, T) is paired with every signal of y --, framed, windowed and transformed
    exactly as stft(params, ., n_fft, hop, win_length=..., center=..., pad_mode=..., detrend=...) does, frames of x and of y side by
    side in one workgroup, and the four sums of welch_csd taken over the frames in the same kernel.  Returns a dict with the `outputs`
    asked for ("pxy", "pxx", "pyy", "coherence", "h1": welch_csd's), each (K,) or (B, K) as y is.  The sums have welch_fft()'s order
    (ascending frames inside chunks of 16, the chunks of a block of 256, then the blocks), so "pxx" / "pyy" are welch_fft of x / of y
    bit for bit, and up to 16 frames every output is welch_csd's bit for bit.  n_fft: a power of two in 16..2048 (ValueError
    otherwise, naming the route that takes 4096, a mixed-radix n_fft or complex input).  `out`: a dict by output name as welch_csd
    takes it; `workspace`: float64, B.csd_fft_workspace_bytes(...) // 8 elements.  With both given the call neither allocates nor
    synchronises and can be captured with no warm call."""
    torch = _torch()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise ValueError("y must be a float32 CUDA tensor")
    return _csd_fft(torch, params, x, y, n_fft, hop, scale, outputs, win_length, center, pad_mode, detrend, onesided_doubling, shift, out,
                    workspace, y.device.index, None)


def _cross_fused(torch, params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, outputs, out, workspace, dev, table, cache):
    B.csd_mask(outputs)
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    L = int(length)
    noverlap = L // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < L:
        raise ValueError("noverlap must be less than length")
    nfft = L if nfft is None else int(nfft)
    hop = L - noverlap
    _csd_fft_input(torch, x, y, nfft, dev)
    if not 1 <= L <= 1 << params.phi_width:
        raise ValueError(f"length {L} outside 1..2^phi_width = {1 << params.phi_width}")
    if nfft < L:
        raise ValueError(f"nfft {nfft} must be at least the window length {L}")
    T = y.shape[-1]
    if T < L or (y.dim() == 2 and y.shape[0] < 1):
        raise ValueError(f"zero segments: T = {T} < length = {L}" if T < L else "zero signals")
    frames = 1 + (T - L) // hop
    xb, yb, nb, bcast, bs = _csd_fft_operands(x, y)
    sums = _window_sums(torch, params, L, True, shift, dev, table, cache)
    scale = B.welch_scale(sums, frames, fs, scaling)
    sh = params.dat_width - 1 if shift is None else int(shift)
    s = B.make_stft(nb, T, frames, hop, nfft, shift=sh, x_stride=bs)
    freqs = _freq_axis(torch, cache, nfft, fs, dev)                    # before the launch: it refuses inside a capture when missing
    res = _csd_fft_call(torch, params, L, s, B.WELCH_DETREND_CONSTANT if detrend == "constant" else 0, xb, yb, nb, nfft // 2 + 1, scale,
                        True, bcast, outputs, out, workspace, dev, table, y.dim() == 1)
    return freqs, res


def cross_spectra_fused(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                        outputs=("pxy", "pxx", "pyy", "coherence", "h1"), out=None, workspace=None):
    """cross_spectra(..., fft="fused") in ONE kernel and a small join (bhw_csd_fft_f32_device): the segments of x and of y, their FFTs
    and the four averages come from the same kernel, so the two (B, F, K) spectra that route writes and reads back never exist.  The
    argument checks, the window sums (cached) and the scale are cross_spectra's for fft="fused"; the estimates are one-sided and only
    the mean is averaged.  Returns (freqs float64, dict by output name); `freqs` is welch_fused's shared, read-only axis.  The sums
    have csd_fft()'s order: equal to cross_spectra(fft="fused") bit for bit up to 16 segments, "pxx" / "pyy" equal to welch_fused of x
    / of y at any length.  Real float32 x and y of the same length, nfft a power of two in 16..2048; anything else is a ValueError
    that names the route that takes it.  After one warm call, with `out` and `workspace` given, it neither synchronises nor allocates
    and can be captured (ResidentTable.cross_spectra_fused); a first call inside a capture raises, as welch_fused does."""
    torch = _torch()
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise ValueError("y must be a float32 CUDA tensor")
    return _cross_fused(torch, params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, outputs, out, workspace, y.device.index,
                        None, _SUMS_CACHE)


def _one_fused(name, f_r):
    return f_r[0], f_r[1][name]


def csd_fused(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None, out=None,
              workspace=None):
    """cross_spectra_fused() with outputs=("pxy",): (freqs, Pxy complex64 (..., K)).  `out`: the tensor itself."""
    return _one_fused("pxy", cross_spectra_fused(params, x, y, fs, length=length, noverlap=noverlap, nfft=nfft, detrend=detrend,
                                                 scaling=scaling, shift=shift, outputs=("pxy",),
                                                 out=None if out is None else {"pxy": out}, workspace=workspace))


def coherence_fused(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                    out=None, workspace=None):
    """cross_spectra_fused() with outputs=("coherence",): (freqs, Cxy float32 (..., K)).  `out`: the tensor itself."""
    return _one_fused("coherence", cross_spectra_fused(params, x, y, fs, length=length, noverlap=noverlap, nfft=nfft, detrend=detrend,
                                                       scaling=scaling, shift=shift, outputs=("coherence",),
                                                       out=None if out is None else {"coherence": out}, workspace=workspace))


def transfer_function_fused(params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                            shift=None, out=None, workspace=None):
    """cross_spectra_fused() with outputs=("h1",): (freqs, H1 complex64 (..., K)).  `out`: the tensor itself."""
    return _one_fused("h1", cross_spectra_fused(params, x, y, fs, length=length, noverlap=noverlap, nfft=nfft, detrend=detrend,
                                                scaling=scaling, shift=shift, outputs=("h1",), out=None if out is None else {"h1": out},
                                                workspace=workspace))


class ResidentTable:
    """A first-quadrant CORDIC table built once and kept on the device (bhw_table_create): the elaboration of win_selector's
    CORDIC from its generics (model, PHI_WIDTH, DAT_WIDTH, PRECISION).  Every call then takes the run-time ports -- the weights
    aa, n_terms, combine -- from its own `params` and reads the same table: no rebuild, no allocation, no synchronisation, so
    the calls can be captured into a graph.  `params` must match the table's generics (BhwError otherwise).  A context manager;
    close() frees the table (after the device has finished with it; a captured graph must not replay it afterwards)."""

    def __init__(self, params, *, device=None, table_format=B.TABLE_BEST):
        torch = _torch()
        self.device = _dev_index(torch, device)
        self.params = B.BhwParams.from_buffer_copy(params)
        h = ctypes.c_void_p()
        B.check(B.lib().bhw_table_create(ctypes.byref(self.params), self.device, _stream_ptr(torch, self.device),
                                         int(table_format), ctypes.byref(h)))
        self.handle = h
        self._sums = {}                      # window sums read back so far (welch)

    def close(self):
        if self.handle:
            B.lib().bhw_table_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        import sys
        if sys.is_finalizing():              # the HIP runtime may already be gone: the process exit frees the table
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.handle:
            raise ValueError("the resident table has been closed")
        return self.handle

    @property
    def nbytes(self):
        """Device bytes the table holds (bhw_table_bytes)."""
        return int(B.lib().bhw_table_bytes(self._live()))

    def describe(self, params, n0, count):
        """The table's format / layout and the kernels generate(params, n0, count) launches (bhw_table_describe)."""
        return B.describe_table(self._live(), params, n0, count)

    def generate(self, params, n0, count, out=None, *, length=None):
        """count coefficients from stream index n0 with params' weights (bhw_generate_from_table), on the current stream.  length:
        the window length L of a window of any length (bhw_generate_len_from_table); None: N = 2^phi_width."""
        torch = _torch()
        h = self._live()
        if out is None:
            out = torch.empty(int(count), dtype=torch.int32, device=f"cuda:{self.device}")
        elif _check_out(torch, out, int(count)) != self.device:
            raise ValueError("out must live on the table's device")
        _call("bhw_generate_from_table", "bhw_generate_len_from_table", (h,), params, length,
              (_stream_ptr(torch, self.device), int(n0), int(count), ctypes.c_void_p(out.data_ptr())))
        return out

    def window(self, params, length, *, sym=False, out=None):
        """window() from this table: the periodic window of `length`, or with sym=True the symmetric one (length >= 2)."""
        length = int(length)
        if sym and length < 2:
            raise ValueError("a symmetric window needs length >= 2")
        return self.generate(params, 0, length, out=out, length=length - 1 if sym else length)

    def apply(self, params, x, n0=0, shift=None, out=None):
        """y[i] = (x[i] * w[n0+i]) >> shift (bhw_apply_from_table); shift defaults to dat_width - 1."""
        torch = _torch()
        h = self._live()
        if x.dtype != torch.int32 or not x.is_cuda or not x.is_contiguous() or x.device.index != self.device:
            raise ValueError("x must be a contiguous int32 CUDA tensor on the table's device")
        if out is None:
            out = torch.empty_like(x)
        elif _check_out(torch, out, x.numel()) != self.device:
            raise ValueError("out must live on the table's device")
        if shift is None:
            shift = params.dat_width - 1
        B.check(B.lib().bhw_apply_from_table(h, ctypes.byref(params), _stream_ptr(torch, self.device), int(n0), x.numel(),
                                             ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), int(shift)))
        return out

    def apply_frames(self, params, x, hop, *, frames=None, channels=1, shift=None, out=None, y_stride=None, length=None):
        """apply_frames() with the coefficients gathered from this table (bhw_apply_frames_from_table, or
        bhw_apply_frames_len_from_table with a length): no allocation by the library, no synchronisation, capturable into a graph."""
        torch = _torch()
        h = self._live()
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device.index != self.device:
            raise ValueError("x must be a contiguous int32 or float32 CUDA tensor on the table's device")
        f, out, result = _frames_call(torch, params, x, int(hop), frames, channels, shift, out, y_stride, self.device, length)
        args = (_stream_ptr(torch, self.device), ctypes.byref(f), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()))
        if x.dtype == torch.float32:
            B.check(B.lib().bhw_apply_frames_f32_from_table(h, ctypes.byref(params), _window_len(params, length), *args))
        else:
            _call("bhw_apply_frames_from_table", "bhw_apply_frames_len_from_table", (h,), params, length, args)
        return result

    def describe_frames(self, params, frames, hop, *, channels=1, y_stride=0):
        """The route and kernels apply_frames(params, ...) launches over this table (bhw_apply_frames_describe)."""
        return B.describe_frames(params, frames, hop, channels=channels, y_stride=y_stride, table=self._live())

    def overlap_add(self, params, y, hop, *, frames=None, channels=1, shift=None, out=None, y_stride=None, t0=0, count=None,
                    length=None, normalize=False):
        """overlap_add() with the coefficients gathered from this table (bhw_overlap_add_from_table, or
        bhw_overlap_add_len_from_table with a length): no allocation by the library, no synchronisation, capturable into a graph."""
        torch = _torch()
        h = self._live()
        if not isinstance(y, torch.Tensor) or not y.is_cuda or y.device.index != self.device:
            raise ValueError("y must be a contiguous int32 or float32 CUDA tensor on the table's device")
        o, out, result, flags = _ola_call(torch, params, y, int(hop), frames, channels, shift, out, y_stride, t0, count, self.device, length,
                                          normalize)
        if y.dtype == torch.float32:
            B.check(B.lib().bhw_overlap_add_f32_from_table(h, ctypes.byref(params), _window_len(params, length), _stream_ptr(torch, self.device),
                                                           ctypes.byref(o), flags, ctypes.c_void_p(y.data_ptr()),
                                                           ctypes.c_void_p(out.data_ptr())))
        else:
            _call("bhw_overlap_add_from_table", "bhw_overlap_add_len_from_table", (h,), params, length,
                  (_stream_ptr(torch, self.device), ctypes.byref(o), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(out.data_ptr())))
        return result

    def describe_overlap_add(self, params, frames, hop, count=None, *, t0=0, channels=1, y_stride=0):
        """The route and kernel overlap_add(params, ...) launches over this table (bhw_overlap_add_describe)."""
        return B.describe_ola(params, frames, hop, count, t0=t0, channels=channels, y_stride=y_stride, table=self._live())

    def stft_frames(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", shift=None, out=None):
        """stft_frames() with the coefficients gathered from this table (bhw_stft_frames_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph."""
        torch = _torch()
        h = self._live()
        s, L, xr, out = _stft_frames_call(torch, params, x, n_fft, hop, win_length, center, pad_mode, shift, out, self.device)
        B.check(B.lib().bhw_stft_frames_f32_from_table(h, ctypes.byref(params), L, _stream_ptr(torch, self.device), ctypes.byref(s),
                                                       ctypes.c_void_p(xr.data_ptr()), ctypes.c_void_p(out.data_ptr())))
        return out

    def stft(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, out=None):
        """stft() with the coefficients gathered from this table (bhw_stft_fft_f32_from_table): no allocation by the library, no
        synchronisation, capturable into a graph on its first call."""
        return _stft(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, out, self.device, self._live())

    def spectrogram(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, fbank=None,
                    shift=None, out=None):
        """spectrogram() with the coefficients gathered from this table (bhw_spectrogram_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph on its first call."""
        return _spectrogram(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, fbank, shift, out, self.device,
                            self._live())

    def stft_mixed(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None, out=None):
        """stft_mixed() with the coefficients gathered from this table (bhw_stft_mfft_f32_from_table): no allocation by the library, no
        synchronisation, capturable into a graph on its first call."""
        return _stft_mixed(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, False, None, shift, out, self.device,
                           self._live())

    def spectrogram_mixed(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, fbank=None,
                          shift=None, out=None):
        """spectrogram_mixed() with the coefficients gathered from this table (bhw_stft_mfft_f32_from_table with BHW_MFFT_POWER): no
        allocation by the library, no synchronisation, capturable into a graph on its first call."""
        return _stft_mixed(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, True, fbank, shift, out, self.device,
                           self._live())

    def stft_iq(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                fftshift=False, out=None):
        """stft_iq() with the coefficients gathered from this table (bhw_stft_cfft_f32_from_table): no allocation by the library, no
        synchronisation, capturable into a graph on its first call."""
        return _stft_iq(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, self.device,
                        self._live(), False)

    def spectrogram_iq(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                       fftshift=False, out=None):
        """spectrogram_iq() with the coefficients gathered from this table (bhw_stft_cfft_f32_from_table with BHW_CFFT_POWER): no
        allocation by the library, no synchronisation, capturable into a graph on its first call."""
        return _stft_iq(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, self.device,
                        self._live(), True)

    def stft_iq_mixed(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                      fftshift=False, out=None):
        """stft_iq_mixed() with the coefficients gathered from this table (bhw_stft_cmfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph on its first call."""
        return _stft_iq(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, self.device,
                        self._live(), False, True)

    def spectrogram_iq_mixed(self, params, x, n_fft, hop, *, win_length=None, center=True, pad_mode="reflect", detrend=False, shift=None,
                             fftshift=False, out=None):
        """spectrogram_iq_mixed() with the coefficients gathered from this table (bhw_stft_cmfft_f32_from_table with BHW_CFFT_POWER):
        no allocation by the library, no synchronisation, capturable into a graph on its first call."""
        return _stft_iq(_torch(), params, x, n_fft, hop, win_length, center, pad_mode, detrend, shift, fftshift, out, self.device,
                        self._live(), True, True)

    def istft(self, params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, out=None):
        """istft() with the coefficients gathered from this table (bhw_istft_fft_f32_from_table): no allocation by the library, no
        synchronisation, capturable into a graph on its first call."""
        return _istft(_torch(), params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, self.device, self._live())

    def istft_mixed(self, params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, out=None):
        """istft_mixed() with the coefficients gathered from this table (bhw_istft_mfft_f32_from_table): no allocation by the library,
        no synchronisation, capturable into a graph on its first call."""
        return _istft(_torch(), params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, self.device, self._live(),
                      _imfft_input)

    def istft_iq(self, params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None, fftshift=False,
                 out=None):
        """istft_iq() with the coefficients gathered from this table (bhw_istft_cfft_f32_from_table): no allocation by the library, no
        synchronisation, capturable into a graph on its first call."""
        torch = _torch()
        return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, self.device, self._live(),
                      _icfft_input, torch.complex64, fftshift)

    def istft_iq_mixed(self, params, Y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None,
                       fftshift=False, out=None):
        """istft_iq_mixed() with the coefficients gathered from this table (bhw_istft_cmfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph on its first call."""
        torch = _torch()
        return _istft(torch, params, Y, n_fft, hop, win_length, center, length, normalize, shift, out, self.device, self._live(),
                      _icmfft_input, torch.complex64, fftshift)

    def istft_overlap_add(self, params, y, n_fft, hop, *, win_length=None, center=True, length=None, normalize=True, shift=None,
                          out=None):
        """istft_overlap_add() with the coefficients gathered from this table (bhw_istft_ola_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph."""
        torch = _torch()
        h = self._live()
        s, L, yr, out, flags = _istft_call(torch, params, y, n_fft, hop, win_length, center, length, normalize, shift, out,
                                           self.device)
        B.check(B.lib().bhw_istft_ola_f32_from_table(h, ctypes.byref(params), L, _stream_ptr(torch, self.device), ctypes.byref(s),
                                                     flags, ctypes.c_void_p(yr.data_ptr()), ctypes.c_void_p(out.data_ptr())))
        return out

    def window_sums(self, params, length, *, f32=False, shift=None):
        """window_sums() with the coefficients gathered from this table (bhw_window_sums_from_table); the numbers are cached on the
        table per (params, length, shift, f32)."""
        return _window_sums(_torch(), params, length, f32, shift, self.device, self._live(), self._sums)

    def welch_frames(self, params, x, length, hop, *, nfft=None, detrend="constant", shift=None, out=None, workspace=None):
        """welch_frames() with the coefficients gathered from this table (bhw_welch_frames_f32_from_table): no allocation by the
        library, no synchronisation, capturable into a graph."""
        return _welch_frames(_torch(), params, x, length, hop, nfft, detrend, shift, out, workspace, self.device, self._live())

    def welch(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
              scaling="density", shift=None, average="mean", fft="torch"):
        """welch() from this table.  The window sums are read back once per (params, length, shift) and kept on the table; after that
        one call the whole chain can be captured into a graph."""
        return _welch(_torch(), params, x, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, average, self.device,
                      self._live(), self._sums, fft)

    def welch_fft(self, params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                  onesided_doubling=True, shift=None, out=None, workspace=None):
        """welch_fft() with the coefficients gathered from this table (bhw_welch_fft_f32_from_table): no allocation by the library,
        no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_fft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift,
                              out, workspace, self.device, self._live())

    def welch_fused(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                    out=None, workspace=None):
        """welch_fused() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can be
        captured into a graph, a first call inside a capture raises."""
        return _welch_fused(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace, self.device,
                            self._live(), self._sums)

    def welch_fft_mixed(self, params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                        onesided_doubling=True, shift=None, out=None, workspace=None):
        """welch_fft_mixed() with the coefficients gathered from this table (bhw_welch_mfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_fft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift,
                              out, workspace, self.device, self._live(), "mfft")

    def welch_fused_mixed(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                          shift=None, out=None, workspace=None):
        """welch_fused_mixed() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can
        be captured into a graph, a first call inside a capture raises."""
        return _welch_fused(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace, self.device,
                            self._live(), self._sums, "mfft")

    def welch_fft_iq(self, params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                     shift=None, fftshift=False, out=None, workspace=None):
        """welch_fft_iq() with the coefficients gathered from this table (bhw_welch_cfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_cfft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, out,
                               workspace, self.device, self._live())

    def welch_fused_iq(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                       shift=None, fftshift=False, out=None, workspace=None):
        """welch_fused_iq() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can be
        captured into a graph, a first call inside a capture raises."""
        return _welch_fused_iq(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, out, workspace,
                               self.device, self._live(), self._sums)

    def welch_fft_iq_mixed(self, params, x, n_fft, hop, scale, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                           shift=None, fftshift=False, out=None, workspace=None):
        """welch_fft_iq_mixed() with the coefficients gathered from this table (bhw_welch_cmfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_cfft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, out,
                               workspace, self.device, self._live(), "cmfft")

    def welch_fused_iq_mixed(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                             shift=None, fftshift=False, out=None, workspace=None):
        """welch_fused_iq_mixed() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call
        can be captured into a graph, a first call inside a capture raises."""
        return _welch_fused_iq(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, out, workspace,
                               self.device, self._live(), self._sums, "cmfft")

    def hold_fft_iq(self, params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                    shift=None, fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fft_iq() with the coefficients gathered from this table (bhw_hold_cfft_f32_from_table): no allocation by the library,
        no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_cfft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, None,
                               workspace, self.device, self._live(), "cfft", (traces, out_max, out_min))

    def hold_fused_iq(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                      fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fused_iq() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can be
        captured into a graph, a first call inside a capture raises."""
        return _welch_fused_iq(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, None, workspace,
                               self.device, self._live(), self._sums, "cfft", (traces, out_max, out_min))

    def hold_fft_iq_mixed(self, params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                          shift=None, fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fft_iq_mixed() with the coefficients gathered from this table (bhw_hold_cmfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_cfft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, shift, fftshift, None,
                               workspace, self.device, self._live(), "cmfft", (traces, out_max, out_min))

    def hold_fused_iq_mixed(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                            shift=None, fftshift=False, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fused_iq_mixed() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call
        can be captured into a graph, a first call inside a capture raises."""
        return _welch_fused_iq(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, fftshift, None, workspace,
                               self.device, self._live(), self._sums, "cmfft", (traces, out_max, out_min))

    def hold_fft(self, params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                 onesided_doubling=True, shift=None, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fft() with the coefficients gathered from this table (bhw_hold_fft_f32_from_table): no allocation by the library, no
        synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_fft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift,
                              None, workspace, self.device, self._live(), "fft", (traces, out_max, out_min))

    def hold_fused(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                   traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fused() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can be
        captured into a graph, a first call inside a capture raises."""
        return _welch_fused(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, None, workspace, self.device,
                            self._live(), self._sums, "fft", (traces, out_max, out_min))

    def hold_fft_mixed(self, params, x, n_fft, hop, scale=1.0, *, win_length=None, center=False, pad_mode="reflect", detrend=False,
                       onesided_doubling=True, shift=None, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fft_mixed() with the coefficients gathered from this table (bhw_hold_mfft_f32_from_table): no allocation by the
        library, no synchronisation, capturable on its first call; the bits are those of the library form."""
        return _welch_fft_psd(_torch(), params, x, n_fft, hop, scale, win_length, center, pad_mode, detrend, onesided_doubling, shift,
                              None, workspace, self.device, self._live(), "mfft", (traces, out_max, out_min))

    def hold_fused_mixed(self, params, x, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                         shift=None, traces="both", out_max=None, out_min=None, workspace=None):
        """hold_fused_mixed() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can
        be captured into a graph, a first call inside a capture raises."""
        return _welch_fused(_torch(), params, x, fs, length, noverlap, nfft, detrend, scaling, shift, None, workspace, self.device,
                            self._live(), self._sums, "mfft", (traces, out_max, out_min))

    def cross_spectra(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                      scaling="density", shift=None, outputs=("pxy", "pxx", "pyy", "coherence", "h1"), fft="torch"):
        """cross_spectra() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the chain can be
        captured into a graph, a first call inside a capture raises."""
        return _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, outputs, self,
                      self._sums, fft)

    def csd(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
            scaling="density", shift=None, fft="torch"):
        """csd() from this table."""
        f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("pxy",), self,
                      self._sums, fft)
        return f, r["pxy"]

    def coherence(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                  scaling="density", shift=None, fft="torch"):
        """coherence() from this table."""
        f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("coherence",), self,
                      self._sums, fft)
        return f, r["coherence"]

    def transfer_function(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", return_onesided=True,
                          scaling="density", shift=None, fft="torch"):
        """transfer_function() from this table."""
        f, r = _cross(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, return_onesided, scaling, shift, ("h1",), self,
                      self._sums, fft)
        return f, r["h1"]

    def csd_fft(self, params, x, y, n_fft, hop, scale, *, outputs=("pxy",), win_length=None, center=False, pad_mode="reflect",
                detrend=False, onesided_doubling=True, shift=None, out=None, workspace=None):
        """csd_fft() with the coefficients gathered from this table (bhw_csd_fft_f32_from_table): no allocation by the library, no
        synchronisation, capturable on its first call; the bits are those of the library form."""
        return _csd_fft(_torch(), params, x, y, n_fft, hop, scale, outputs, win_length, center, pad_mode, detrend, onesided_doubling,
                        shift, out, workspace, self.device, self._live())

    def cross_spectra_fused(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                            shift=None, outputs=("pxy", "pxx", "pyy", "coherence", "h1"), out=None, workspace=None):
        """cross_spectra_fused() from this table.  The sums cache and the capture rule are welch()'s: after one warm call the call can
        be captured into a graph, a first call inside a capture raises."""
        return _cross_fused(_torch(), params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, outputs, out, workspace,
                            self.device, self._live(), self._sums)

    def _one_fused(self, name, params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace):
        f, r = self.cross_spectra_fused(params, x, y, fs, length=length, noverlap=noverlap, nfft=nfft, detrend=detrend, scaling=scaling,
                                        shift=shift, outputs=(name,), out=None if out is None else {name: out}, workspace=workspace)
        return f, r[name]

    def csd_fused(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density", shift=None,
                  out=None, workspace=None):
        """csd_fused() from this table."""
        return self._one_fused("pxy", params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace)

    def coherence_fused(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                        shift=None, out=None, workspace=None):
        """coherence_fused() from this table."""
        return self._one_fused("coherence", params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace)

    def transfer_function_fused(self, params, x, y, fs=1.0, *, length, noverlap=None, nfft=None, detrend="constant", scaling="density",
                                shift=None, out=None, workspace=None):
        """transfer_function_fused() from this table."""
        return self._one_fused("h1", params, x, y, fs, length, noverlap, nfft, detrend, scaling, shift, out, workspace)

    def generate_part(self, params, part, n_parts, window):
        """Interleaved ownership part `part` of `n_parts` into the full-length `window` (bhw_generate_part_from_table)."""
        torch = _torch()
        h = self._live()
        if _check_out(torch, window, 1 << params.phi_width, "window") != self.device:
            raise ValueError("window must live on the table's device")
        B.check(B.lib().bhw_generate_part_from_table(h, ctypes.byref(params), _stream_ptr(torch, self.device), int(part),
                                                     int(n_parts), ctypes.c_void_p(window.data_ptr())))
        return window


def generate_batched(params, frames, *, device=None, out=None):
    """frames x 2^phi_width coefficients: one period computed, then replicated (bhw_generate_batched_device)."""
    torch = _torch()
    dev = _dev_index(torch, device)
    n = 1 << params.phi_width
    if out is None:
        out = torch.empty((int(frames), n), dtype=torch.int32, device=f"cuda:{dev}")
    dev = _check_out(torch, out, int(frames) * n)
    B.check(B.lib().bhw_generate_batched_device(ctypes.byref(params), dev, _stream_ptr(torch, dev), int(frames),
                                                 ctypes.c_void_p(out.data_ptr())))
    return out


def cordic(params, theta0, count, *, device=None):
    """(sin, cos) int32 CUDA tensors for phases theta0..theta0+count-1 (bhw_sincos_device)."""
    torch = _torch()
    dev = _dev_index(torch, device)
    s = torch.empty(int(count), dtype=torch.int32, device=f"cuda:{dev}")
    c = torch.empty(int(count), dtype=torch.int32, device=f"cuda:{dev}")
    B.check(B.lib().bhw_sincos_device(ctypes.byref(params), dev, _stream_ptr(torch, dev), int(theta0), int(count),
                                       ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(c.data_ptr())))
    return s, c


def atan2(x, y, *, PRECISION=1, INPUT_WIDTH=20, ANGLE_WIDTH=16, out=None):
    """entity cordic_atan2 (src/cordic_atan2.vhd:64-76) over int32 CUDA tensors VEC_DX = x, VEC_DY = y: returns PHI_DT
    (ANGLE_WIDTH-bit words, sign-extended; full circle = 2^ANGLE_WIDTH) via bhw_atan2_device."""
    torch = _torch()
    if x.dtype != torch.int32 or y.dtype != torch.int32 or not x.is_cuda or x.device != y.device or x.shape != y.shape:
        raise ValueError("x and y must be int32 CUDA tensors of the same shape on one device")
    x, y = x.contiguous(), y.contiguous()
    dev = x.device.index
    phi = torch.empty_like(x) if out is None else out
    if phi.dtype != torch.int32 or phi.device != x.device or phi.numel() != x.numel() or not phi.is_contiguous():
        raise ValueError("out must be a contiguous int32 tensor like x")
    p = B.BhwAtan2Params(ctypes.sizeof(B.BhwAtan2Params), PRECISION, INPUT_WIDTH, ANGLE_WIDTH)
    B.check(B.lib().bhw_atan2_device(ctypes.byref(p), dev, _stream_ptr(torch, dev), x.numel(),
                                      ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                      ctypes.c_void_p(phi.data_ptr())))
    return phi


def win_function(win_type, i0, count, *, nphase, nwidth, device=None, **kw):
    """HLS top function swept over i (hls/windows/win_function.h:65-69): unknown win_type -> zeros
    (win_empty, hls/windows/win_function.cpp:159-165,417-419)."""
    torch = _torch()
    if win_type not in (1, 2, 3, 4, 5, 7):
        return torch.zeros(int(count), dtype=torch.int32, device="cuda" if device is None else device)
    p = B.make_params(win_type, nphase, nwidth, model=B.MODEL_HLS, combine=B.COMBINE_HLS, **kw)
    return generate(p, i0, count, device=device)


class WinSelector:
    """entity win_selector (src/win_selector.vhd:60-87).

    Generics become constructor arguments with the reference's names; the AA0..AA6 ports are the
    `aa` list (integer, caller-scaled; None = the HLS model's built-in constants).  `model`/`combine`
    choose which of the reference's bit-models to reproduce (default: the HLS C++ model).
    """

    def __init__(self, PHI_WIDTH=10, DAT_WIDTH=16, WIN_TYPE="HAMMING", SIN_TYPE="CORDIC", LUT_SIZE=9,
                 XSERIES="ULTRA", aa=None, model=B.MODEL_HLS, combine=B.COMBINE_HLS, precision=1, device=None):
        if WIN_TYPE not in _WIN_TYPES:
            raise ValueError(f"WIN_TYPE {WIN_TYPE!r}: expected one of {sorted(_WIN_TYPES)}")
        if SIN_TYPE not in ("CORDIC", "TAYLOR", "TAYLOR_ALL"):
            raise ValueError("SIN_TYPE must be 'CORDIC' or 'TAYLOR' (or this library's extension 'TAYLOR_ALL')")
        if XSERIES not in ("7SERIES", "ULTRA"):  # selects DSP48 port widths only (tay1_order.vhd:538-578)
            raise ValueError("XSERIES must be '7SERIES' or 'ULTRA'")
        self.device = device
        self.params = B.make_params(
            _WIN_TYPES[WIN_TYPE], PHI_WIDTH, DAT_WIDTH, model=model, combine=combine,
            sin_type=self._sin_type(SIN_TYPE, _WIN_TYPES[WIN_TYPE]),
            precision=precision, lut_size=LUT_SIZE, aa=aa)
        self._phase = 0  # the PHI_WIDTH-bit counter (RESET clears it: bh_win_7term.vhd:179-186)
        self._table = None  # ResidentTable of the generics after elaborate()

    @staticmethod
    def _sin_type(SIN_TYPE, win_type):
        """The selector hands SIN_TYPE only to hamming_win and bh_win_3term (src/win_selector.vhd:93-135); the 4/5/7-term
        entities have no such generic (:137-199), so "TAYLOR" there still elaborates the CORDIC design.  "TAYLOR_ALL" is
        the extension of include/bhw.h (Taylor source for every term count)."""
        if SIN_TYPE == "TAYLOR_ALL":
            return B.SIN_TAYLOR_ALL
        if SIN_TYPE == "TAYLOR" and win_type in (1, 2, 3):
            return B.SIN_TAYLOR
        return B.SIN_CORDIC

    @property
    def length(self):
        return 1 << self.params.phi_width

    def reset(self):
        self._phase = 0

    def elaborate(self, table_format=B.TABLE_BEST):
        """Build the CORDIC table of the generics once (ResidentTable) -- what elaboration does for the entity.  Afterwards
        enable / apply / window / shard(layout="interleaved") read it, and a change of self.params.aa between calls is a change
        on the AA ports: it takes effect from the next call, with no rebuild.  Nothing to keep for the Taylor source (its ROM is
        cached by the library): a no-op there."""
        if self.params.sin_type != B.SIN_CORDIC or self._table is not None:
            return self
        self._table = ResidentTable(self.params, device=self.device, table_format=table_format)
        return self

    def release(self):
        """Free the table elaborate() built (the calls go back to the per-call table)."""
        if self._table is not None:
            self._table.close()
            self._table = None

    @property
    def table(self):
        """The ResidentTable after elaborate(), else None."""
        return self._table

    def enable(self, count, out=None, algo=B.ALGO_AUTO):
        """ENABLE high for `count` clocks: the next `count` values of DT_WIN; the counter advances and wraps."""
        if self._table is not None and algo == B.ALGO_AUTO:
            w = self._table.generate(self.params, self._phase, count, out=out)
            self._phase = (self._phase + int(count)) % self.length
            return w
        w = generate(self.params, self._phase, count, device=self.device, out=out, algo=algo)
        self._phase = (self._phase + int(count)) % self.length
        return w

    def apply(self, x, shift=None, out=None):
        """The multiplier stage behind DT_WIN for the next x.numel() clocks: y = (x * DT_WIN) >> shift."""
        if self._table is not None:
            y = self._table.apply(self.params, x, n0=self._phase, shift=shift, out=out)
            self._phase = (self._phase + x.numel()) % self.length
            return y
        y = apply(self.params, x, n0=self._phase, shift=shift, out=out)
        self._phase = (self._phase + x.numel()) % self.length
        return y

    def window(self, out=None, algo=B.ALGO_AUTO):
        """One full period from phase 0."""
        if self._table is not None and algo == B.ALGO_AUTO:
            return self._table.generate(self.params, 0, self.length, out=out)
        return generate(self.params, 0, self.length, device=self.device, out=out, algo=algo)

    def shard(self, rank, world_size, out=None, algo=B.ALGO_AUTO, layout="contiguous"):
        """This rank's share of ONE window over `world_size` devices, no collective.
        layout "contiguous": the index range shard_range(N, rank, world_size), returned as a tensor of that length.
        layout "interleaved": the ownership part (rank, world_size) of include/bhw.h -- ring lanes with their eight quadrant /
        half-period images, so the folds still share CORDIC work; written into `out`, a full-length window buffer (allocated
        when None: elements this rank does not own stay uninitialised), which is returned; self.segments(...) lists them."""
        if layout == "contiguous":
            n0, count = shard_range(self.length, rank, world_size)
            return generate(self.params, n0, count, device=self.device, out=out, algo=algo)
        if layout != "interleaved":
            raise ValueError("layout must be 'contiguous' or 'interleaved'")
        if out is None:
            torch = _torch()
            out = torch.empty(self.length, dtype=torch.int32, device=f"cuda:{_dev_index(torch, self.device)}")
        if self._table is not None and self._table_parts_ok() and algo == B.ALGO_AUTO:
            return self._table.generate_part(self.params, rank, world_size, out)
        return generate_part(self.params, rank, world_size, out, algo=algo)

    def _table_parts_ok(self):
        """Parts come from the table where it is in the tile layout (phi_width >= 22); shorter windows' parts are the fused
        kernel's and need no table."""
        return self.params.phi_width >= 22

    def segments(self, rank, world_size):
        """[(n0, count), ...] owned by `rank` in the interleaved layout (host arithmetic, no GPU needed)."""
        return B.part_segments(self.params, rank, world_size)
