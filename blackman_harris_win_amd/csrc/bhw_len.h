// bhw_len.h -- the phase map of windows of any length L (the *_len entry points of include/bhw.h), shared by the HIP-free planner
// (bhw_plan.cpp) and the kernels (bhw_device.h).
//
// A power-of-two window reads harmonic k of coefficient n at the angle theta_k = (k * n) mod 2^P: the phase accumulator counts modulo
// 2^PHI_WIDTH.  A window of length L, 1 <= L <= 2^P, reads it at the nearest phi_width-bit angle of the exact one:
//     m = n mod L,  m_k = (k * m) mod L,  theta_k = round(m_k * 2^P / L) mod 2^P
// At L = 2^P this is (k * n) mod 2^P with no rounding.  With L = 2^a * b (b odd, a <= P) a tie would need 2^(P + 1 - a) * m_k = b
// (mod 2b): even against odd, so rounding never meets a tie (half up and half to even agree, and theta_k(L - m) = -theta_k(m)).
//
// theta_k = floor((m_k * 2^(P+1) + L) / 2L): m_k < L <= 2^30 and P <= 30 keep the numerator below 2^62.  The division by 2L is a
// 64-bit multiply-high by the host-computed reciprocal floor((2^64 - 1) / 2L) and one correction (the estimate is the quotient or
// one less), so no kernel divides.  m_k follows m_{k-1} by an add and a compare (bhw_len_step): k * m is never formed.
#pragma once
#include <cstdint>

struct BhwLenPhase {
    uint64_t len;        // L
    uint64_t inv2l;      // floor((2^64 - 1) / (2L))
    uint32_t pw;         // P = phi_width
    uint32_t reserved;
};

inline BhwLenPhase bhw_len_phase(uint32_t phi_width, uint64_t length)
{
    return BhwLenPhase{length, ~0ull / (2u * length), phi_width, 0u};
}

BHW_HD inline uint64_t bhw_len_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(x / 2L) and x mod 2L for any 64-bit x
BHW_HD inline uint64_t bhw_len_div2l(uint64_t x, const BhwLenPhase &lp, uint64_t &rem)
{
    const uint64_t d = 2u * lp.len;
    uint64_t q = bhw_len_mulhi(x, lp.inv2l);
    uint64_t r = x - q * d;
    if (r >= d) {
        ++q;
        r -= d;
    }
    rem = r;
    return q;
}

// n mod L for any 64-bit n
BHW_HD inline uint64_t bhw_len_mod(uint64_t n, const BhwLenPhase &lp)
{
    uint64_t r;
    (void)bhw_len_div2l(n, lp, r);
    return r >= lp.len ? r - lp.len : r;
}

// theta = round(mk * 2^P / L) mod 2^P for 0 <= mk < L
BHW_HD inline uint32_t bhw_len_theta(uint64_t mk, const BhwLenPhase &lp)
{
    uint64_t r;
    const uint64_t q = bhw_len_div2l((mk << (lp.pw + 1u)) + lp.len, lp, r);
    return (uint32_t)q & ((1u << lp.pw) - 1u);
}

// m_k = (m_{k-1} + m) mod L, for m, m_{k-1} < L
BHW_HD inline uint64_t bhw_len_step(uint64_t mk, uint64_t m, const BhwLenPhase &lp)
{
    mk += m;
    return mk >= lp.len ? mk - lp.len : mk;
}
