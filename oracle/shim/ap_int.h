/* Stand-in for the arbitrary-width integer header the HLS sources of the reference include ("ap_int.h").
 * The project's own code, written from the rules below and from nothing else; test infrastructure only (oracle/Makefile
 * compiles the reference's HLS sources against it into oracle/_ref).  Its self-test is tests/cpp/san_ap_int_shim.cpp.
 *
 * The contract: compute exactly, wrap on every store.
 *
 *  1. ap_int<W> is signed, ap_uint<W> unsigned, 1 <= W <= 127.  A value is kept in a signed __int128, always inside the type's
 *     range: [-2^(W-1), 2^(W-1)) or [0, 2^W).
 *  2. Constructing or assigning from a built-in integer, from a double (truncated toward zero first) or from another
 *     ap_[u]int<V> reduces the value modulo 2^W; a signed type then sign-extends from bit W-1.
 *  3. + - * & | ^, the comparisons and == between two such values, or between one and a built-in integer, are evaluated on the
 *     128-bit values and give an ap_int<127>: no bit is lost before the next store.  (The vendor's result types grow by one bit
 *     for + and -, and to the sum of the widths for *; a 127-bit result holds every one of them that these sources produce.)
 *     Why 128 bits suffice for NWIDTH <= 32: the widest intermediate of the HLS sources is dbl_t * win_t,
 *     (2 NWIDTH + 1) + NWIDTH = 3 NWIDTH + 1 = 97 bits at NWIDTH 32; every sum of such products stays below 2^100.
 *  4. x >> n has the width and signedness of x; for a signed x it is the arithmetic shift (floor(x / 2^n)).
 *  5. x << n has the WIDTH OF x: bits shifted past W are lost (and bit W-1 becomes the sign of a signed type).
 *  6. ~x has the width and signedness of x.
 *  7. Unary minus is 0 - x (rule 3).
 *
 * Undefined behaviour is kept out by construction: all wrapping arithmetic runs in unsigned __int128, no negative value is ever
 * shifted, and the way back to the signed representation negates a non-negative number.  (Only the conversion from a double
 * outside the 128-bit range would be undefined; these sources convert weights below 2^32.)
 *
 * Nothing else belongs here: no fixed point, no bit ranges, no streams.
 */
#ifndef BHW_ORACLE_SHIM_AP_INT_H
#define BHW_ORACLE_SHIM_AP_INT_H

#include <type_traits>

namespace ap_shim {

typedef __int128 i128;
typedef unsigned __int128 u128;

/* two's-complement reading of 128 bits, without an out-of-range conversion */
constexpr i128 as_signed(u128 u) { return (u >> 127) ? -(i128)(~u) - 1 : (i128)u; }

/* rule 2: reduce modulo 2^W, sign-extend for a signed type */
template <int W, bool S> constexpr i128 wrap(u128 u) {
    const u128 mask = (((u128)1) << W) - 1;                 /* W <= 127 */
    u &= mask;
    if (S && ((u >> (W - 1)) & 1)) u |= ~mask;
    return as_signed(u);
}

/* floor(v / 2^n) without shifting a negative value */
constexpr i128 shr(i128 v, int n) {
    if (n <= 0) return v;
    if (n > 127) n = 127;
    return v < 0 ? ~((~v) >> n) : v >> n;
}

template <int W, bool S> struct ap_base {
    static_assert(W >= 1 && W <= 127, "ap_[u]int<W>: 1 <= W <= 127 (values are kept in __int128)");
    i128 v;

    constexpr ap_base() : v(0) {}
    template <class T, class = typename std::enable_if<std::is_integral<T>::value || std::is_same<T, i128>::value ||
                                                       std::is_same<T, u128>::value>::type>
    constexpr ap_base(T x) : v(wrap<W, S>((u128)x)) {}
    constexpr ap_base(double d) : v(wrap<W, S>((u128)(i128)d)) {}
    template <int V, bool T> constexpr ap_base(const ap_base<V, T> &o) : v(wrap<W, S>((u128)o.v)) {}

    constexpr ap_base operator>>(int n) const { return ap_base(shr(v, n)); }
    constexpr ap_base operator<<(int n) const {
        if (n <= 0) return *this;
        if (n >= W) return ap_base(0);
        return ap_base((u128)v << n);
    }
    constexpr ap_base operator~() const { return ap_base(-v - 1); }     /* |v| < 2^127: no overflow */
    constexpr ap_base<127, true> operator-() const;
    /* the way out to built-in integers (the callers of the HLS functions need one): the low 64 bits, as a store to ap_int<64> */
    explicit constexpr operator long long() const { return (long long)wrap<64, true>((u128)v); }
};

typedef ap_base<127, true> wide;

constexpr i128 val(i128 x) { return x; }
template <int W, bool S> constexpr i128 val(const ap_base<W, S> &x) { return x.v; }

template <class T> struct is_ap : std::false_type {};
template <int W, bool S> struct is_ap<ap_base<W, S> > : std::true_type {};
template <class T> struct is_int : std::integral_constant<bool, std::is_integral<T>::value> {};
/* an operator takes part when at least one side is an ap value and the other is an ap value or a built-in integer */
template <class A, class B> struct mixes
    : std::integral_constant<bool, (is_ap<A>::value && (is_ap<B>::value || is_int<B>::value)) || (is_int<A>::value && is_ap<B>::value)> {};

#define AP_SHIM_ARITH(OP)                                                                                          \
    template <class A, class B, class = typename std::enable_if<mixes<A, B>::value>::type>                         \
    constexpr wide operator OP(const A &a, const B &b) {                                                           \
        return wide((u128)val(a) OP (u128)val(b));                                                                 \
    }
AP_SHIM_ARITH(+)
AP_SHIM_ARITH(-)
AP_SHIM_ARITH(*)
AP_SHIM_ARITH(&)
AP_SHIM_ARITH(|)
AP_SHIM_ARITH(^)
#undef AP_SHIM_ARITH

#define AP_SHIM_COMPARE(OP)                                                                                        \
    template <class A, class B, class = typename std::enable_if<mixes<A, B>::value>::type>                         \
    constexpr bool operator OP(const A &a, const B &b) {                                                           \
        return val(a) OP val(b);                                                                                   \
    }
AP_SHIM_COMPARE(<)
AP_SHIM_COMPARE(>)
AP_SHIM_COMPARE(<=)
AP_SHIM_COMPARE(>=)
AP_SHIM_COMPARE(==)
AP_SHIM_COMPARE(!=)
#undef AP_SHIM_COMPARE

template <int W, bool S> constexpr wide ap_base<W, S>::operator-() const { return 0 - *this; }

}  // namespace ap_shim

template <int W> using ap_int = ap_shim::ap_base<W, true>;
template <int W> using ap_uint = ap_shim::ap_base<W, false>;

#endif
