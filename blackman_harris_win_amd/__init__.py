"""blackman_harris_win_amd -- MI355X-native fixed-point window-coefficient generator.

Python host side above the C ABI of include/bhw.h.  PyTorch supplies device memory, streams and
torch.distributed only; every coefficient is computed by the hand-written HIP kernels in
libbhw.so.  There is no CPU compute path here: if the library is missing or no GPU is present,
the compute calls raise.

The surface mirrors the reference's operator:
  * ``WinSelector``  <->  entity win_selector (src/win_selector.vhd:60-87): generics PHI_WIDTH,
    DAT_WIDTH, WIN_TYPE, SIN_TYPE, LUT_SIZE and weight ports AA0..AA6; ``enable(count)`` is
    "hold ENABLE high for count clocks" and returns DT_WIN.
  * ``win_function(win_type, i0, count, ...)``  <->  HLS top win_function(win_type, i, &out)
    (hls/windows/win_function.h:65-69) swept over i.
  * ``cordic(theta0, count, ...)``  <->  cordic() (cpp/cordic_sincos.cpp:10, hls/cordic/cordic.cpp:45).
"""
from .binding import (  # noqa: F401
    ALGO_AUTO, ALGO_DIRECT, ALGO_FUSED, ALGO_TABLE,
    TABLE_BEST, TABLE_DELTA16, TABLE_NIBBLE, TABLE_NIBBLE_ESC, TABLE_PLAIN, TABLE_RESIDUAL,
    COMBINE_HLS, COMBINE_VHDL,
    MODEL_CPP, MODEL_DDS48, MODEL_HLS, MODEL_SCALED, MODEL_VHDL,
    SIN_CORDIC, SIN_TAYLOR, SIN_TAYLOR_ALL,
    WIN_BH3, WIN_BH4, WIN_BH5, WIN_BH7, WIN_HAMMING, WIN_HANN,
    BhwAtan2Params, BhwError, BhwFrames, BhwOla, BhwParams, BhwPsd, BhwCsd, BhwStft, WELCH_BLOCK, WELCH_FFT_CHUNK, describe_welch_fft, welch_fft_workspace_bytes, describe_csd_fft, csd_fft_workspace_bytes, describe_stft_cmfft, describe_mask_fft, describe_mask_mfft, describe_cmask_fft, describe_cmask_mfft, describe_mask_cfft, describe_cmask_cfft, describe_mask_cmfft, describe_cmask_cmfft, describe_beam_fft, describe_beam_mfft, BEAM_MAX_CH, describe_welch_cfft, welch_cfft_workspace_bytes, describe_welch_mfft, welch_mfft_workspace_bytes, describe_welch_cmfft, welch_cmfft_workspace_bytes, describe_hold_cfft, hold_cfft_workspace_bytes, describe_hold_cmfft, hold_cmfft_workspace_bytes, describe_hold_fft, hold_fft_workspace_bytes, describe_hold_mfft, hold_mfft_workspace_bytes, describe_welch, describe_csd, PAD_CONSTANT, PAD_REFLECT, coeffs_from_float, describe_f32, describe_frames, describe_len, describe_ola, describe_stft, describe_stft_fft, describe_istft_fft, describe_spectrogram, describe_stft_mfft, describe_istft_mfft, mfft_supported, MFFT_POWER, describe_stft_cfft, describe_istft_cfft, describe_istft_cmfft, make_fbank, BhwFbank, BhwLogspec, make_logspec, describe_logspec, describe_logspec_mfft, LOG_CLAMP, LOG_ADD, constant_tables, describe_table, lib, lib_path, make_params, part_segments,
)
from .selector import (  # noqa: F401
    ResidentTable, WinSelector, apply, apply_frames, atan2, istft_overlap_add, stft, istft, spectrogram, stft_mixed, spectrogram_mixed, istft_mixed, stft_iq, spectrogram_iq, stft_iq_mixed, spectrogram_iq_mixed, istft_iq, istft_iq_mixed, stft_mask_istft, stft_mask_istft_mixed, stft_cmask_istft, stft_cmask_istft_mixed, stft_mask_istft_iq, stft_cmask_istft_iq, stft_mask_istft_iq_mixed, stft_cmask_istft_iq_mixed, stft_beamform_istft, stft_beamform_istft_mixed, FilterBank, mel_weights, DctMatrix, dct_weights, log_spectrogram, log_spectrogram_mixed, mfcc, mfcc_mixed, stft_frames, welch, welch_fft, welch_fused, welch_fft_iq, welch_fused_iq, welch_fft_mixed, welch_fused_mixed, welch_fft_iq_mixed, welch_fused_iq_mixed, hold_fft_iq, hold_fused_iq, hold_fft_iq_mixed, hold_fused_iq_mixed, hold_fft, hold_fused, hold_fft_mixed, hold_fused_mixed, welch_frames, welch_psd, welch_csd, csd, coherence, transfer_function, cross_spectra, csd_fft, cross_spectra_fused, csd_fused, coherence_fused, transfer_function_fused, window_sums, overlap_add, cordic, gather_parts, generate, generate_batched, generate_part, prepare, shard_range, win_function, window,
)

__all__ = [
    "WinSelector", "ResidentTable", "win_function", "cordic", "atan2", "generate", "generate_batched", "generate_part", "gather_parts", "part_segments", "apply",
    "apply_frames", "describe_frames", "overlap_add", "describe_ola", "window", "describe_len", "describe_f32",
    "stft_frames", "istft_overlap_add", "describe_stft", "stft", "describe_stft_fft", "istft", "describe_istft_fft",
    "spectrogram", "FilterBank", "mel_weights", "describe_spectrogram", "make_fbank",
    "stft_mixed", "spectrogram_mixed", "describe_stft_mfft", "mfft_supported", "MFFT_POWER",
    "istft_mixed", "describe_istft_mfft",
    "log_spectrogram", "log_spectrogram_mixed", "mfcc", "mfcc_mixed", "DctMatrix", "dct_weights", "describe_logspec",
    "describe_logspec_mfft", "make_logspec",
    "stft_iq", "spectrogram_iq", "describe_stft_cfft", "istft_iq", "describe_istft_cfft",
    "stft_iq_mixed", "spectrogram_iq_mixed", "describe_stft_cmfft", "istft_iq_mixed", "describe_istft_cmfft",
    "stft_mask_istft", "describe_mask_fft", "stft_mask_istft_mixed", "describe_mask_mfft",
    "stft_cmask_istft", "describe_cmask_fft", "stft_cmask_istft_mixed", "describe_cmask_mfft",
    "stft_mask_istft_iq", "describe_mask_cfft", "stft_cmask_istft_iq", "describe_cmask_cfft",
    "stft_mask_istft_iq_mixed", "describe_mask_cmfft", "stft_cmask_istft_iq_mixed", "describe_cmask_cmfft",
    "stft_beamform_istft", "describe_beam_fft", "stft_beamform_istft_mixed", "describe_beam_mfft", "BEAM_MAX_CH",
    "window_sums", "welch_frames", "welch_psd", "welch", "describe_welch",
    "welch_fft", "welch_fused", "describe_welch_fft", "welch_fft_workspace_bytes", "WELCH_FFT_CHUNK",
    "welch_fft_iq", "welch_fused_iq", "describe_welch_cfft", "welch_cfft_workspace_bytes",
    "welch_fft_mixed", "welch_fused_mixed", "describe_welch_mfft", "welch_mfft_workspace_bytes",
    "welch_fft_iq_mixed", "welch_fused_iq_mixed", "describe_welch_cmfft", "welch_cmfft_workspace_bytes",
    "hold_fft_iq", "hold_fused_iq", "describe_hold_cfft", "hold_cfft_workspace_bytes",
    "hold_fft_iq_mixed", "hold_fused_iq_mixed", "describe_hold_cmfft", "hold_cmfft_workspace_bytes",
    "hold_fft", "hold_fused", "describe_hold_fft", "hold_fft_workspace_bytes",
    "hold_fft_mixed", "hold_fused_mixed", "describe_hold_mfft", "hold_mfft_workspace_bytes",
    "welch_csd", "csd", "coherence", "transfer_function", "cross_spectra", "describe_csd",
    "csd_fft", "cross_spectra_fused", "csd_fused", "coherence_fused", "transfer_function_fused", "describe_csd_fft", "csd_fft_workspace_bytes",
    "prepare", "shard_range",
    "make_params", "coeffs_from_float", "constant_tables", "BhwParams", "BhwError", "lib", "lib_path",
]
