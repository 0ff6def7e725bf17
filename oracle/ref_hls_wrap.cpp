/* extern "C" entry points around the reference's HLS functions.  The project's own code: oracle/Makefile appends this file to
 * the translation unit it streams to the compiler (the reference's header, then its source, then this), so NPHASE, NWIDTH,
 * phi_t, win_t / out_t and the functions called below are the reference's.  REF_HLS_CORDIC_ONLY is defined for
 * hls/cordic/cordic.cpp, which has cordic() alone and names its output type out_t.
 *
 * Single-threaded on purpose: the reference's cordic() refills a static table on every call, so it must not be entered from
 * two threads.  A caller that wants more cores starts more processes.
 */
#include <stdint.h>

#ifdef REF_HLS_CORDIC_ONLY
typedef out_t ref_out_t;
#else
typedef win_t ref_out_t;
#endif

extern "C" {

void ref_hls_widths(int *nphase, int *nwidth) {
    *nphase = NPHASE;
    *nwidth = NWIDTH;
}

/* (sin, cos) of the phases theta0 .. theta0 + count - 1, each reduced modulo 2^NPHASE by the phi_t store */
void ref_hls_sincos(uint64_t theta0, uint64_t count, int32_t *sin, int32_t *cos) {
    for (uint64_t i = 0; i < count; i++) {
        ref_out_t c, s;
        cordic(phi_t((unsigned long long)(theta0 + i)), &c, &s);
        sin[i] = (int32_t)(long long)s;
        cos[i] = (int32_t)(long long)c;
    }
}

#ifndef REF_HLS_CORDIC_ONLY
/* coefficients n0 .. n0 + count - 1 of window win_type; an unknown win_type gives zeros (the reference's win_empty) */
void ref_hls_window(int win_type, uint64_t n0, uint64_t count, int32_t *out) {
    for (uint64_t i = 0; i < count; i++) {
        win_t o;
        win_function((char)win_type, phi_t((unsigned long long)(n0 + i)), &o);
        out[i] = (int32_t)(long long)o;
    }
}
#endif

}
