// The exponential of the gradient-boosting unit (solver_gb.hip), HIP-free: IEEE +, -, *, /, rint and ldexp only, so the
// device, the host and NumPy (tests/gb_restated.py mirrors it line for line) give the same bits for the same argument.
// The unit is compiled -ffp-contract=off: no product below is fused into a sum.
//   * the argument is clamped to [-708, 708]: both ends stay normal numbers, and 1 / (1 + gb_exp(708)) is a normal number
//   * Cody-Waite reduction by ln 2 in two parts (fdlibm's constants: the high part has 21 trailing zero bits, so k * hi is
//     exact for |k| <= 1022): x = k ln 2 + r, |r| <= ln 2 / 2
//   * the Taylor polynomial of degree 13 in Horner form (the first dropped term is below 2^-57 of the result)
//   * ldexp(p, k): a multiplication by a power of two, exact here
// Its distance from the C library's exp: DESIGN.md section 5 (measured by tests/test_gb_host.py on NumPy's mirror).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GB_HD __host__ __device__
#else
#define GB_HD
#endif

GB_HD inline double gb_exp(double x)
{
    if (x > 708.0) x = 708.0;
    if (x < -708.0) x = -708.0;
    const double k = rint(x * 0x1.71547652b82fep+0);
    const double r = (x - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
    double q = 0x1.6124613a86d09p-33;          // 1 / 13!
    q = q * r + 0x1.1eed8eff8d898p-29;         // 1 / 12!
    q = q * r + 0x1.ae64567f544e4p-26;         // 1 / 11!
    q = q * r + 0x1.27e4fb7789f5cp-22;         // 1 / 10!
    q = q * r + 0x1.71de3a556c734p-19;         // 1 / 9!
    q = q * r + 0x1.a01a01a01a01ap-16;         // 1 / 8!
    q = q * r + 0x1.a01a01a01a01ap-13;         // 1 / 7!
    q = q * r + 0x1.6c16c16c16c17p-10;         // 1 / 6!
    q = q * r + 0x1.1111111111111p-7;          // 1 / 5!
    q = q * r + 0x1.5555555555555p-5;          // 1 / 4!
    q = q * r + 0x1.5555555555555p-3;          // 1 / 3!
    q = q * r + 0x1.0000000000000p-1;          // 1 / 2!
    q = q * r + 1.0;
    q = q * r + 1.0;
    return ldexp(q, (int)k);
}

// scikit-learn's expit of the raw prediction, through gb_exp
GB_HD inline double gb_expit(double x) { return 1.0 / (1.0 + gb_exp(-x)); }
