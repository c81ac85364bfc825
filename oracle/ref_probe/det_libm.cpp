/*
 * oracle/ref_probe/det_libm.cpp -- TEST INFRASTRUCTURE.
 *
 * The transcendental functions the reference's path code calls, defined on top
 * of oracle/det_math.h and linked into path_probe in front of libm, so that the
 * reference's own instructions run with the oracle's polynomials.  sincosf is
 * among them because GCC fuses cos(x) and sin(x) of one argument into one
 * sincosf call, -fno-builtin or not.  oracle/Makefile checks with nm -D that
 * the probe imports none of these families from libm.
 */
#include "../det_math.h"

extern "C" {
float cosf(float x) noexcept { return om_cosf(x); }
float sinf(float x) noexcept { return om_sinf(x); }
float tanf(float x) noexcept { return om_tanf(x); }
float acosf(float x) noexcept { return om_acosf(x); }
float atan2f(float y, float x) noexcept { return om_atan2f(y, x); }
float expf(float x) noexcept { return om_expf(x); }
float log10f(float x) noexcept { return om_log10f(x); }
float powf(float x, float y) noexcept { return om_powf(x, y); }
void sincosf(float x, float* s, float* c) noexcept
{
    *s = om_sinf(x);
    *c = om_cosf(x);
}
}
