// bhw.hpp -- C++ host mirror of the reference's operator interface, header-only, on top of the C ABI (bhw.h).
//
// The reference is compiled code (VHDL entities + C++ bit-models), so the host side above the ABI is C++:
//   bhw::win_selector   <->  entity win_selector            src/win_selector.vhd:60-87
//   bhw::win_function() <->  HLS top win_function()         hls/windows/win_function.h:65-69
//   bhw::cordic()       <->  cordic()                       cpp/cordic_sincos.cpp:10, hls/cordic/cordic.cpp:45;
//                            entities cordic_dds / cordic_dds48 / cordic_dds_scaled (model BHW_MODEL_VHDL / _DDS48 / _SCALED)
//   bhw::cordic_atan2() <->  entity cordic_atan2            src/cordic_atan2.vhd:64-76
//   bhw::resident_table      the elaborated CORDIC of win_selector's generics (bhw_table_create), move-only, RAII
//   bhw::apply_frames()      the window over overlapping frames of a signal in one launch (bhw_apply_frames_device)
//   bhw::overlap_add()       the weighted overlap-add of frames back into one signal in one launch (bhw_overlap_add_device)
//   bhw::generate_len(), bhw::apply_frames_len(), bhw::overlap_add_len()
//                            the same for a window of any length L <= 2^phi_width (bhw_generate_len_device ...)
//   bhw::apply_frames_f32(), bhw::overlap_add_f32()
//                            float32 samples, with the envelope division of the overlap-add (bhw_apply_frames_f32_device ...)
//   bhw::stft_frames_f32(), bhw::istft_ola_f32()
//                            the framing of torch.stft / torch.istft for a batch (centred, padded, win_length < n_fft)
// Same names, argument meaning and error behaviour (unknown win_type -> zeros, like win_empty,
// hls/windows/win_function.cpp:159-165,417-419).  All arithmetic runs in the HIP kernels behind the ABI.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "bhw.h"

namespace bhw {

struct error : std::runtime_error {
    int code;
    error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc)
{
    if (rc != BHW_OK) throw error(rc, std::string(bhw_strerror(rc)) + ": " + bhw_last_error());
}

// entity win_selector: generics become constructor arguments under the reference's names.
class win_selector {
public:
    win_selector(unsigned PHI_WIDTH, unsigned DAT_WIDTH, const std::string &WIN_TYPE, const std::string &SIN_TYPE = "CORDIC",
                 unsigned LUT_SIZE = 9, const std::string &XSERIES = "ULTRA", int device = 0)
        : device_(device)
    {
        uint32_t wt = 0;
        if (WIN_TYPE == "HAMMING") wt = BHW_WIN_HAMMING;
        else if (WIN_TYPE == "HANN") wt = BHW_WIN_HANN;
        else if (WIN_TYPE == "BH3TERM") wt = BHW_WIN_BH3;
        else if (WIN_TYPE == "BH4TERM") wt = BHW_WIN_BH4;
        else if (WIN_TYPE == "BH5TERM") wt = BHW_WIN_BH5;
        else if (WIN_TYPE == "BH7TERM") wt = BHW_WIN_BH7;
        else throw error(BHW_ERR_BADARG, "WIN_TYPE " + WIN_TYPE);
        if (XSERIES != "ULTRA" && XSERIES != "7SERIES") throw error(BHW_ERR_BADARG, "XSERIES " + XSERIES);
        int rc = bhw_params_init(&p_, wt, PHI_WIDTH, DAT_WIDTH);
        if (rc != BHW_OK && p_.n_terms == 0) check(rc);
        // SIN_TYPE reaches only hamming_win and bh_win_3term (src/win_selector.vhd:93-135); the 4/5/7-term entities have
        // no such generic (:137-199), so "TAYLOR" there is still the CORDIC design.  "TAYLOR_ALL": extension, see bhw.h.
        if (SIN_TYPE == "TAYLOR_ALL") p_.sin_type = BHW_SIN_TAYLOR_ALL;
        else if (SIN_TYPE == "TAYLOR") p_.sin_type = (p_.n_terms <= 3) ? BHW_SIN_TAYLOR : BHW_SIN_CORDIC;
        else if (SIN_TYPE != "CORDIC") throw error(BHW_ERR_BADARG, "SIN_TYPE " + SIN_TYPE);
        p_.lut_size = LUT_SIZE;
        check(bhw_params_validate(&p_));
    }

    // the AA0..AA6 ports (integer, caller-scaled)
    void set_AA(const std::vector<int32_t> &aa)
    {
        for (size_t k = 0; k < 7; ++k) p_.aa[k] = k < aa.size() ? aa[k] : 0;
    }
    void set_model(uint32_t model, uint32_t combine, uint32_t precision = 1)
    {
        p_.model = model;
        p_.combine = combine;
        p_.precision = precision;
        check(bhw_params_validate(&p_));
    }
    void RESET() { phase_ = 0; }
    uint64_t length() const { return 1ull << p_.phi_width; }

    // ENABLE high for `count` clocks: the next `count` values of DT_WIN into device memory (async on `stream`).
    void ENABLE(uint64_t count, int32_t *d_out, void *stream = nullptr)
    {
        check(bhw_generate_device(&p_, device_, stream, phase_, count, d_out));
        phase_ = (phase_ + count) % length();
    }
    // same, delivered to host memory
    std::vector<int32_t> ENABLE(uint64_t count)
    {
        std::vector<int32_t> v(count);
        check(bhw_generate_to_host(&p_, device_, phase_, count, v.data()));
        phase_ = (phase_ + count) % length();
        return v;
    }
    // the multiplier stage behind DT_WIN: d_y[i] = (d_x[i] * DT_WIN) >> shift for the next `count` clocks
    void APPLY(uint64_t count, const int32_t *d_x, int32_t *d_y, unsigned shift, void *stream = nullptr)
    {
        check(bhw_apply_device(&p_, device_, stream, phase_, count, d_x, d_y, shift));
        phase_ = (phase_ + count) % length();
    }
    // Every lazy step of later calls done now (ROM upload, scratch, packed-table verification): bhw_prepare_device.
    void PREPARE(void *stream = nullptr) { check(bhw_prepare_device(&p_, device_, stream)); }
    // One window over several devices without a collective: what part `part` of `n_parts` owns ...
    std::vector<bhw_segment> SEGMENTS(uint32_t part, uint32_t n_parts) const
    {
        uint32_t n = 0;
        check(bhw_part_segments(&p_, part, n_parts, nullptr, 0, &n));
        std::vector<bhw_segment> v(n);
        check(bhw_part_segments(&p_, part, n_parts, v.data(), n, &n));
        return v;
    }
    // ... and those coefficients written into d_window, the base of a full-length (2^PHI_WIDTH) device buffer
    void ENABLE_PART(uint32_t part, uint32_t n_parts, int32_t *d_window, void *stream = nullptr)
    {
        check(bhw_generate_part_device(&p_, device_, stream, part, n_parts, d_window, nullptr));
    }
    // the whole window on this selector's device from its n_parts parts (d_windows[g] on src_devices[g]): peer copies of the
    // owned segments, no collective (bhw_gather_parts_device)
    void GATHER_PARTS(uint32_t n_parts, const int *src_devices, const int32_t *const *d_windows, int32_t *d_dst, void *stream = nullptr)
    {
        check(bhw_gather_parts_device(&p_, n_parts, src_devices, d_windows, device_, stream, d_dst));
    }
    // AA0..AA6 from one of the named coefficient sets of the reference's comments / README (bhw_coeffs_preset); the window
    // type must be the preset's
    void AA_PRESET(uint32_t preset)
    {
        uint32_t wt = 0;
        int32_t aa[7];
        check(bhw_coeffs_preset(preset, p_.dat_width, &wt, nullptr, aa));
        if (wt != p_.win_type) throw error(BHW_ERR_BADARG, "preset belongs to another window type");
        for (int k = 0; k < 7; ++k) p_.aa[k] = aa[k];
    }
    const bhw_params &params() const { return p_; }

private:
    bhw_params p_{};
    uint64_t phase_ = 0;
    int device_;
};

// HLS top swept over i = i0 .. i0+count-1.
inline std::vector<int32_t> win_function(char win_type, uint64_t i0, uint64_t count, unsigned NPHASE, unsigned NWIDTH, int device = 0)
{
    std::vector<int32_t> v(count, 0);
    bhw_params p;
    if (bhw_params_init(&p, (uint32_t)(unsigned char)win_type, NPHASE, NWIDTH) != BHW_OK) {
        if (p.n_terms == 0) return v;  // win_empty
        check(bhw_params_validate(&p));
    }
    check(bhw_generate_to_host(&p, device, i0, count, v.data()));
    return v;
}

// cordic() swept over theta: returns {sin, cos} vectors.  model = BHW_MODEL_CPP reproduces cpp/cordic_sincos.cpp.
inline void cordic(uint32_t model, unsigned PHASE_WIDTH, unsigned DATA_WIDTH, uint64_t theta0, uint64_t count,
                   std::vector<int32_t> &s, std::vector<int32_t> &c, int device = 0)
{
    bhw_params p;
    bhw_params_init(&p, BHW_WIN_HAMMING, PHASE_WIDTH, DATA_WIDTH);
    p.model = model;
    s.resize(count);
    c.resize(count);
    check(bhw_sincos_to_host(&p, device, theta0, count, s.data(), c.data()));
}

// entity cordic_atan2 (src/cordic_atan2.vhd:64-76) over host vectors VEC_DX, VEC_DY -> PHI_DT.
inline std::vector<int32_t> cordic_atan2(unsigned PRECISION, unsigned INPUT_WIDTH, unsigned ANGLE_WIDTH,
                                         const std::vector<int32_t> &VEC_DX, const std::vector<int32_t> &VEC_DY, int device = 0)
{
    if (VEC_DX.size() != VEC_DY.size()) throw error(BHW_ERR_BADARG, "VEC_DX / VEC_DY lengths differ");
    bhw_atan2_params p{(uint32_t)sizeof(bhw_atan2_params), PRECISION, INPUT_WIDTH, ANGLE_WIDTH};
    std::vector<int32_t> phi(VEC_DX.size());
    check(bhw_atan2_to_host(&p, device, VEC_DX.size(), VEC_DX.data(), VEC_DY.data(), phi.data()));
    return phi;
}

// The descriptor of an overlapped-frame apply: `frames` frames of `hop` time indices apart, `channels` 1 or 2 (I/Q), y_stride 0 = N * C.
inline bhw_frames frames(uint64_t n_frames, uint64_t hop, uint32_t shift, uint32_t channels = 1, uint64_t y_stride = 0)
{
    return bhw_frames{(uint32_t)sizeof(bhw_frames), channels, n_frames, hop, y_stride, shift, 0u};
}

// Overlapped-frame apply (the STFT / Welch front end): the window of `p` over every frame of d_x in one launch
// (bhw_apply_frames_device); device pointers and stream as in the C call.
inline void apply_frames(const bhw_params &p, const bhw_frames &f, const int32_t *d_x, int32_t *d_y, int device = 0, void *hip_stream = nullptr)
{
    check(bhw_apply_frames_device(&p, device, hip_stream, &f, d_x, d_y));
}

// The descriptor of a weighted overlap-add: `frames` frames of `hop` time indices apart summed into the outputs [t0, t0 + count),
// `channels` 1 or 2 (I/Q), y_stride 0 = N * C.
inline bhw_ola ola(uint64_t n_frames, uint64_t hop, uint64_t count, uint32_t shift, uint64_t t0 = 0, uint32_t channels = 1,
                   uint64_t y_stride = 0)
{
    return bhw_ola{(uint32_t)sizeof(bhw_ola), channels, n_frames, hop, y_stride, t0, count, shift, 0u};
}

// Weighted overlap-add (the STFT synthesis side): every frame of d_y windowed by `p` again and summed into d_x in one launch
// (bhw_overlap_add_device); device pointers and stream as in the C call.
inline void overlap_add(const bhw_params &p, const bhw_ola &o, const int32_t *d_y, int32_t *d_x, int device = 0, void *hip_stream = nullptr)
{
    check(bhw_overlap_add_device(&p, device, hip_stream, &o, d_y, d_x));
}

// Windows of any length L, 1 <= L <= 2^phi_width (the *_len calls of bhw.h): count coefficients of the length-L window from index n0
// into device memory, the overlapped-frame apply and the overlap-add with L in place of N, and the one-line route description
// (f / o NULL: the generate call).
inline void generate_len(const bhw_params &p, uint64_t length, uint64_t n0, uint64_t count, int32_t *d_out, int device = 0,
                         void *hip_stream = nullptr)
{
    check(bhw_generate_len_device(&p, length, device, hip_stream, n0, count, d_out));
}
inline void apply_frames_len(const bhw_params &p, uint64_t length, const bhw_frames &f, const int32_t *d_x, int32_t *d_y, int device = 0,
                             void *hip_stream = nullptr)
{
    check(bhw_apply_frames_len_device(&p, length, device, hip_stream, &f, d_x, d_y));
}
inline void overlap_add_len(const bhw_params &p, uint64_t length, const bhw_ola &o, const int32_t *d_y, int32_t *d_x, int device = 0,
                            void *hip_stream = nullptr)
{
    check(bhw_overlap_add_len_device(&p, length, device, hip_stream, &o, d_y, d_x));
}
inline std::string describe_len(const bhw_params &p, uint64_t length, uint64_t n0, uint64_t count, const bhw_frames *f = nullptr,
                                const bhw_ola *o = nullptr, bhw_table t = nullptr)
{
    char buf[512];
    check(bhw_describe_len(t, &p, length, n0, count, f, o, buf, sizeof buf));
    return buf;
}

// Float32 frame apply and overlap-add over the window of length L (2^phi_width: the power-of-two window): v[k] = fl32(w[k]) * 2^-shift
// applied to float32 samples; flags BHW_OLA_NORMALIZE divides each output by the window envelope (bhw.h gives the arithmetic), and
// the one-line description (exactly one of f and o).
inline void apply_frames_f32(const bhw_params &p, uint64_t length, const bhw_frames &f, const float *d_x, float *d_y, int device = 0,
                             void *hip_stream = nullptr)
{
    check(bhw_apply_frames_f32_device(&p, length, device, hip_stream, &f, d_x, d_y));
}
inline void overlap_add_f32(const bhw_params &p, uint64_t length, const bhw_ola &o, uint32_t flags, const float *d_y, float *d_x,
                            int device = 0, void *hip_stream = nullptr)
{
    check(bhw_overlap_add_f32_device(&p, length, device, hip_stream, &o, flags, d_y, d_x));
}
inline std::string describe_f32(const bhw_params &p, uint64_t length, const bhw_frames *f, const bhw_ola *o, uint32_t flags = 0,
                                bhw_table t = nullptr)
{
    char buf[512];
    check(bhw_describe_f32(t, &p, length, f, o, flags, buf, sizeof buf));
    return buf;
}

// Batched, centred STFT framing and overlap-add over the window of length L (bhw.h gives the arithmetic): one launch per side for the
// B signals of the descriptor, and the one-line description (inverse: the overlap-add).
inline void stft_frames_f32(const bhw_params &p, uint64_t length, const bhw_stft &s, const float *d_x, float *d_y, int device = 0,
                            void *hip_stream = nullptr)
{
    check(bhw_stft_frames_f32_device(&p, length, device, hip_stream, &s, d_x, d_y));
}
inline void istft_ola_f32(const bhw_params &p, uint64_t length, const bhw_stft &s, uint32_t flags, const float *d_y, float *d_x,
                          int device = 0, void *hip_stream = nullptr)
{
    check(bhw_istft_ola_f32_device(&p, length, device, hip_stream, &s, flags, d_y, d_x));
}
inline std::string describe_stft(const bhw_params &p, uint64_t length, const bhw_stft &s, bool inverse, uint32_t flags = 0,
                                 bhw_table t = nullptr)
{
    char buf[640];
    check(bhw_describe_stft(t, &p, length, &s, inverse ? 1 : 0, flags, buf, sizeof buf));
    return buf;
}

// The CORDIC table of a configuration's generics, built once on `device` (bhw_table_create) and freed by the destructor
// (bhw_table_destroy: it synchronises the device first).  Move-only.  Every call takes its weights -- the AA ports -- from its own
// bhw_params, which must match the table's generics; device pointers and streams as in the C calls.
class resident_table {
public:
    resident_table() = default;
    explicit resident_table(const bhw_params &p, int device = 0, void *hip_stream = nullptr, uint32_t table_format = BHW_TABLE_BEST)
    {
        check(bhw_table_create(&p, device, hip_stream, table_format, &t_));
    }
    ~resident_table() { bhw_table_destroy(t_); }
    resident_table(const resident_table &) = delete;
    resident_table &operator=(const resident_table &) = delete;
    resident_table(resident_table &&o) noexcept : t_(o.t_) { o.t_ = nullptr; }
    resident_table &operator=(resident_table &&o) noexcept
    {
        if (this != &o) {
            bhw_table_destroy(t_);
            t_ = o.t_;
            o.t_ = nullptr;
        }
        return *this;
    }

    bhw_table get() const { return t_; }
    explicit operator bool() const { return t_ != nullptr; }
    uint64_t bytes() const { return bhw_table_bytes(t_); }
    std::string describe(const bhw_params &p, uint64_t n0, uint64_t count) const
    {
        char buf[384];
        check(bhw_table_describe(t_, &p, n0, count, buf, sizeof buf));
        return buf;
    }
    void generate(const bhw_params &p, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out) const
    {
        check(bhw_generate_from_table(t_, &p, hip_stream, n0, count, d_out));
    }
    void apply(const bhw_params &p, void *hip_stream, uint64_t n0, uint64_t count, const int32_t *d_x, int32_t *d_y, uint32_t shift) const
    {
        check(bhw_apply_from_table(t_, &p, hip_stream, n0, count, d_x, d_y, shift));
    }
    void apply_frames(const bhw_params &p, void *hip_stream, const bhw_frames &f, const int32_t *d_x, int32_t *d_y) const
    {
        check(bhw_apply_frames_from_table(t_, &p, hip_stream, &f, d_x, d_y));
    }
    std::string describe_frames(const bhw_params &p, const bhw_frames &f) const
    {
        char buf[384];
        check(bhw_apply_frames_describe(t_, &p, &f, buf, sizeof buf));
        return buf;
    }
    void overlap_add(const bhw_params &p, void *hip_stream, const bhw_ola &o, const int32_t *d_y, int32_t *d_x) const
    {
        check(bhw_overlap_add_from_table(t_, &p, hip_stream, &o, d_y, d_x));
    }
    std::string describe_overlap_add(const bhw_params &p, const bhw_ola &o) const
    {
        char buf[384];
        check(bhw_overlap_add_describe(t_, &p, &o, buf, sizeof buf));
        return buf;
    }
    // windows of any length L from this table (bhw_generate_len_from_table ...)
    void generate_len(const bhw_params &p, uint64_t length, void *hip_stream, uint64_t n0, uint64_t count, int32_t *d_out) const
    {
        check(bhw_generate_len_from_table(t_, &p, length, hip_stream, n0, count, d_out));
    }
    void apply_frames_len(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_frames &f, const int32_t *d_x, int32_t *d_y) const
    {
        check(bhw_apply_frames_len_from_table(t_, &p, length, hip_stream, &f, d_x, d_y));
    }
    void overlap_add_len(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_ola &o, const int32_t *d_y, int32_t *d_x) const
    {
        check(bhw_overlap_add_len_from_table(t_, &p, length, hip_stream, &o, d_y, d_x));
    }
    std::string describe_len(const bhw_params &p, uint64_t length, uint64_t n0, uint64_t count, const bhw_frames *f = nullptr,
                             const bhw_ola *o = nullptr) const
    {
        return bhw::describe_len(p, length, n0, count, f, o, t_);
    }
    // float32 samples from this table (bhw_apply_frames_f32_from_table ...)
    void apply_frames_f32(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_frames &f, const float *d_x, float *d_y) const
    {
        check(bhw_apply_frames_f32_from_table(t_, &p, length, hip_stream, &f, d_x, d_y));
    }
    void overlap_add_f32(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_ola &o, uint32_t flags, const float *d_y,
                         float *d_x) const
    {
        check(bhw_overlap_add_f32_from_table(t_, &p, length, hip_stream, &o, flags, d_y, d_x));
    }
    std::string describe_f32(const bhw_params &p, uint64_t length, const bhw_frames *f, const bhw_ola *o, uint32_t flags = 0) const
    {
        return bhw::describe_f32(p, length, f, o, flags, t_);
    }
    // batched STFT framing and overlap-add from this table (bhw_stft_frames_f32_from_table ...)
    void stft_frames_f32(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_stft &s, const float *d_x, float *d_y) const
    {
        check(bhw_stft_frames_f32_from_table(t_, &p, length, hip_stream, &s, d_x, d_y));
    }
    void istft_ola_f32(const bhw_params &p, uint64_t length, void *hip_stream, const bhw_stft &s, uint32_t flags, const float *d_y,
                       float *d_x) const
    {
        check(bhw_istft_ola_f32_from_table(t_, &p, length, hip_stream, &s, flags, d_y, d_x));
    }
    std::string describe_stft(const bhw_params &p, uint64_t length, const bhw_stft &s, bool inverse, uint32_t flags = 0) const
    {
        return bhw::describe_stft(p, length, s, inverse, flags, t_);
    }
    void generate_part(const bhw_params &p, void *hip_stream, uint32_t part, uint32_t n_parts, int32_t *d_window) const
    {
        check(bhw_generate_part_from_table(t_, &p, hip_stream, part, n_parts, d_window));
    }

private:
    bhw_table t_ = nullptr;
};

} // namespace bhw
