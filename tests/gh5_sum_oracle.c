/* The oracle's GF(2^128) multiply for tests/gh5_sum_host.cc: gf128_mul is a
 * file-local function of oracle/qpp_oracle.c, so that file is compiled into
 * this unit and the one function handed on. */
#include "../oracle/qpp_oracle.c"

void gh5_sum_gf128(uint8_t x[16], const uint8_t y[16]) { gf128_mul(x, y); }
