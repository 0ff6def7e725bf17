// Self-test of oracle/shim/ap_int.h (the project's stand-in for the header the reference's HLS sources include), built with
// -fsanitize=address,undefined by tests/test_ap_int_shim.py.  Every check holds the contract written at the top of that header
// against plain unsigned __int128 arithmetic or against constants worked out by hand / in Python integers.  Prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <cstdint>

#include "ap_int.h"

typedef __int128 i128;
typedef unsigned __int128 u128;

static long checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++checks;                                                            \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static i128 pow2(int n) { return (i128)((u128)1 << n); }   // n <= 126

// value of the low W bits of u, read as unsigned / as two's complement: the rule of the header, restated with % and compares
static i128 expect_unsigned(u128 u, int W) { return (i128)(u % ((u128)1 << W)); }
static i128 expect_signed(u128 u, int W) {
    i128 r = expect_unsigned(u, W);
    return r >= pow2(W - 1) ? (W == 127 ? r - pow2(126) - pow2(126) : r - pow2(W)) : r;
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {      // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static u128 rnd128() { return ((u128)rnd64() << 64) | rnd64(); }

template <int W> static void wrap_at_width() {
    const i128 lo = -pow2(W - 1), hi = pow2(W - 1) - 1;
    const i128 umax = pow2(W - 1) + hi;                       // 2^W - 1 without forming 2^127
    // the edges: 2^(W-1) - 1 stays, 2^(W-1) wraps to the minimum, the minimum stays, minimum - 1 wraps to the maximum
    CHECK(ap_int<W>(hi).v == hi);
    CHECK(ap_int<W>(lo).v == lo);
    CHECK(ap_int<W>(-1).v == -1);
    CHECK(ap_uint<W>(-1).v == umax);
    CHECK(ap_uint<W>(0).v == 0 && ap_int<W>(0).v == 0);
    if (W < 127) {
        CHECK(ap_int<W>(hi + 1).v == lo);
        CHECK(ap_int<W>(lo - 1).v == hi);
        CHECK(ap_uint<W>(pow2(W)).v == 0);
        CHECK(ap_uint<W>(pow2(W) + 5).v == 5 % pow2(W));
        CHECK(ap_uint<W>(pow2(W) - 1).v == pow2(W) - 1);
        CHECK(ap_int<W>(pow2(W) + pow2(W - 1)).v == lo);
    }
    // sign extension: bit W-1 alone is the minimum of the signed type and 2^(W-1) of the unsigned one
    CHECK(ap_int<W>((u128)1 << (W - 1)).v == lo);
    CHECK(ap_uint<W>((u128)1 << (W - 1)).v == (i128)((u128)1 << (W - 1)));
    for (int i = 0; i < 2000; i++) {
        u128 u = rnd128();
        if (i & 1) u >>= (rnd64() % 128);
        ap_int<W> s(u);
        ap_uint<W> z(u);
        CHECK(s.v == expect_signed(u, W));
        CHECK(z.v == expect_unsigned(u, W));
        CHECK(s.v >= lo && s.v <= hi && z.v >= 0);
        // a store from another width reduces the same way, whichever type carried the value
        ap_int<127> wide_s(u);
        ap_uint<127> wide_u(u);
        CHECK(ap_int<W>(wide_s).v == s.v && ap_int<W>(wide_u).v == s.v);
        CHECK(ap_uint<W>(wide_s).v == z.v && ap_uint<W>(wide_u).v == z.v);
        ap_int<W> assigned;
        assigned = (long long)(uint64_t)u;
        CHECK(assigned.v == expect_signed((u128)(i128)(long long)(uint64_t)u, W));
        // ~x + 1 == -x after a store, and ~x is the W-bit complement
        ap_int<W> neg = ~s + 1;
        CHECK(neg.v == expect_signed((u128)0 - (u128)s.v, W));
        CHECK(neg.v == ap_int<W>(-s).v);
        CHECK((~s).v == -s.v - 1);
        CHECK((~z).v == umax - z.v);
        // >> : floor division, the width of the left operand; << : bits past W are lost
        int n = (int)(rnd64() % (W + 3 < 127 ? W + 3 : 127));                   // past the width too, where 126 allows
        i128 fl = s.v >= 0 ? s.v / pow2(n) : -((-(s.v + 1)) / pow2(n)) - 1;     // floor(s / 2^n) by division
        CHECK((s >> n).v == fl);
        CHECK((z >> n).v == z.v / pow2(n));
        CHECK((s << n).v == (n >= W ? 0 : expect_signed((u128)s.v << n, W)));
        CHECK((z << n).v == (n >= W ? 0 : expect_unsigned((u128)z.v << n, W)));
    }
}

int main() {
    wrap_at_width<1>();
    wrap_at_width<2>();
    wrap_at_width<8>();
    wrap_at_width<10>();
    wrap_at_width<34>();
    wrap_at_width<65>();
    wrap_at_width<127>();

    // W = 1 and 2 by hand
    CHECK(ap_int<1>(1).v == -1 && ap_int<1>(2).v == 0 && ap_int<1>(3).v == -1 && ap_uint<1>(3).v == 1);
    CHECK(ap_int<2>(2).v == -2 && ap_int<2>(3).v == -1 && ap_int<2>(5).v == 1 && ap_uint<2>(7).v == 3 && ap_uint<2>(-2).v == 2);
    CHECK(ap_int<8>(128).v == -128 && ap_int<8>(255).v == -1 && ap_int<8>(-129).v == 127 && ap_uint<8>(256 + 7).v == 7);
    CHECK(ap_int<10>(512).v == -512 && ap_int<10>(1023).v == -1 && ap_uint<10>(1024 + 1023).v == 1023);

    // << drops bits at the width of its LEFT operand; + and * lose none before the store
    {
        ap_int<10> a(0x155);                       // 01 0101 0101
        CHECK((a << 1).v == -342);                 // 10 1010 1010 as ten signed bits
        CHECK((a << 2).v == 0x154);                // 01 0101 0100: the top bit fell off
        CHECK((a << 9).v == -512 && (a << 10).v == 0 && (a << 40).v == 0);
        ap_int<34> wide = a << 2;                  // the bits were lost at 10 bits, before the wider store
        CHECK(wide.v == 0x154);
        ap_int<34> wide2 = ap_int<34>(a) << 2;     // widened first: nothing lost
        CHECK(wide2.v == 0x554);
        ap_uint<8> u(0xC3);
        CHECK((u << 1).v == 0x86 && (u << 7).v == 0x80 && (u << 8).v == 0);
        ap_int<10> m(511);
        ap_int<34> sum = m + m;                    // 1022 needs 11 bits: kept until the store
        CHECK(sum.v == 1022);
        ap_int<10> sum10 = m + m;
        CHECK(sum10.v == -2);
        ap_int<34> prod = m * m;
        CHECK(prod.v == 261121);
        ap_int<10> prod10 = m * m;                 // 261121 mod 1024 = 1
        CHECK(prod10.v == 1);
        ap_int<10> mn(-512);
        ap_int<34> diff = mn - m;
        CHECK(diff.v == -1023);
        CHECK((mn - 1).v == -513 && (1 - mn).v == 513 && (2 * mn).v == -1024 && (mn * 2).v == -1024);
        ap_int<10> twice = 2 * m;                  // the 2 * i of the window functions: wraps only at the phi_t store
        CHECK(twice.v == -2);
    }

    // >> of negative values: arithmetic
    {
        ap_int<10> a(-1), b(-512), c(-5);
        CHECK((a >> 1).v == -1 && (a >> 9).v == -1 && (a >> 100).v == -1);
        CHECK((b >> 8).v == -2 && (b >> 9).v == -1 && (b >> 1).v == -256);
        CHECK((c >> 1).v == -3 && (c >> 2).v == -2 && (c >> 0).v == -5);
        ap_int<65> d(-(((i128)1) << 64));
        CHECK((d >> 63).v == -2 && (d >> 64).v == -1 && (d >> 3).v == -(((i128)1) << 61));
        ap_uint<10> e(-1);
        CHECK((e >> 9).v == 1 && (e >> 10).v == 0);
        // ap_uint<2> built from a negative ap_int<10> >> 8: the quadrant of the upper half of the circle
        ap_int<10> q2(-512), q2b(-257), q3(-256), q3b(-1), q0(255), q1(256);
        CHECK(ap_uint<2>(q2 >> 8).v == 2 && ap_uint<2>(q2b >> 8).v == 2);
        CHECK(ap_uint<2>(q3 >> 8).v == 3 && ap_uint<2>(q3b >> 8).v == 3);
        CHECK(ap_uint<2>(q0 >> 8).v == 0 && ap_uint<2>(q1 >> 8).v == 1);
        ap_uint<2> quadrant = q3 >> 8;
        CHECK(quadrant == 0x3 && !(quadrant == 0x0) && quadrant == 3u);
    }

    // ~x + 1 == -x after a store; the minimum is its own negative
    {
        ap_int<34> x(123456789), mn(-(((i128)1) << 33));
        ap_int<34> nx = ~x + 1, nmn = ~mn + 1;
        CHECK(nx.v == -123456789 && nmn.v == mn.v && (~x).v == -123456790);
        CHECK((~x + 1).v == -123456789);           // before the store as well
        CHECK((~mn + 1).v == (((i128)1) << 33));   // exact before the store: 2^33 does not fit 34 signed bits, the store wraps it
        ap_uint<8> u(5);
        CHECK((~u).v == 250 && ap_uint<8>(~u + 1).v == 251);
        CHECK((3 & ~ap_int<10>(1)).v == 2 && (ap_int<10>(-1) & 0xFF).v == 255 && (ap_int<10>(-1) & ~(0x3 << 8)).v == -769);
        CHECK((ap_int<10>(5) | 2).v == 7 && (ap_int<10>(5) ^ ap_uint<8>(1)).v == 4);
    }

    // double construction truncates toward zero, then wraps
    {
        CHECK(ap_int<65>(2147483647.0).v == 2147483647 && ap_int<65>(-2147483647.0).v == -2147483647);
        CHECK(ap_int<32>(2147483647.0).v == 2147483647 && ap_int<32>(-2147483647.0).v == -2147483647);
        CHECK(ap_int<31>(2147483647.0).v == -1 && ap_int<31>(-2147483647.0).v == 1);
        CHECK(ap_int<65>(4611686018427387904.0).v == (((i128)1) << 62));
        CHECK(ap_int<63>(4611686018427387904.0).v == -(((i128)1) << 62) && ap_uint<62>(4611686018427387904.0).v == 0);
        CHECK(ap_int<34>(1234.75).v == 1234 && ap_int<34>(-1234.75).v == -1234 && ap_int<34>(0.99).v == 0 && ap_int<34>(-0.99).v == 0);
        CHECK(ap_int<8>(300.9).v == 44 && ap_uint<8>(-1.5).v == 255);
        ap_int<65> a0 = 291220644.0;               // a weight as the window functions store it
        CHECK(a0.v == 291220644);
    }

    // a 65-bit x 32-bit product (dbl_t * win_t at NWIDTH 32), exact until the store
    {
        ap_int<65> a(-(((i128)1) << 64));          // the minimum of 65 bits
        ap_int<32> c(-2147483647 - 1);
        CHECK((a * c).v == (((i128)1) << 95));     // 2^64 * 2^31
        CHECK(((a * c) >> 30).v == (((i128)1) << 65));
        ap_int<65> stored = (a * c) >> 30;         // 2^65 mod 2^65
        CHECK(stored.v == 0);
        ap_int<65> b((((i128)1) << 64) - 1);
        ap_int<32> d(2147483647);
        // (2^64 - 1)(2^31 - 1) = 2^95 - 2^64 - 2^31 + 1 = 39614081238685424727874437121 (Python integers)
        i128 want = ((i128)1 << 95) - ((i128)1 << 64) - ((i128)1 << 31) + 1;
        CHECK((b * d).v == want && (d * b).v == want);
        CHECK(((b * d) >> 30).v == ((i128)1 << 65) - ((i128)1 << 34) - 2);       // floor(want / 2^30)
        CHECK((a * d).v == -(((i128)1 << 95) - ((i128)1 << 64)));
        CHECK(((a * d) >> 30).v == -(((i128)1 << 65) - ((i128)1 << 34)));
        ap_int<65> acc = 291220644.0;
        ap_int<32> out = (ap_int<32>)(acc - ((ap_int<65>(465407608) * ap_int<32>(1073741823)) >> 30));
        CHECK(out.v == 291220644 - 465407607);     // floor(465407608 * (2^30 - 1) / 2^30) = 465407607
    }

    // comparisons on the exact values, across widths and signedness
    {
        ap_int<10> a(-1);
        ap_uint<10> b(1023);
        CHECK(a < 0 && !(b < 0) && a < b && b > a && a != b && !(a == b) && a <= -1 && a >= -1 && 0 > a);
        CHECK(ap_int<10>(b) == a && ap_uint<10>(a) == b);
        CHECK((long long)a == -1 && (long long)b == 1023);
    }

    std::printf("ok %ld\n", checks);
    return 0;
}
