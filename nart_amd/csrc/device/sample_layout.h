// What the LatinSquare and splat kernels (kernels.h) and the host's plans of their launches
// (host/latin_plan.h, host/splat_plan.h) share, as plain C++ that compiles with and without HIP: the
// read-ahead and padding sizes that decide how far the LatinSquare scratch arrays lie apart, and the
// sizes of the splat's filter-cell table and lane groups.  tests/test_latin_plan.py and
// tests/test_splat_plan.py check the arithmetic built on them on the CPU.
#pragma once

// ---------------------------------------------------------------- LatinSquare in three kernels
// k_latin_draws / k_latin_emit: slots of one k_latin_emit block; the states st are u32
// [slot / LATIN_EMIT_SLOTS][k][slot % LATIN_EMIT_SLOTS]
#define LATIN_EMIT_SLOTS 16
#define LATIN_ST_PAD (256 * 8 * 4)  // words read past the last block's states by k_latin_emit

#ifndef NART_LATIN_PF
#define NART_LATIN_PF 16  // choice words (2 swaps each) loaded one batch ahead of their swaps
#endif

// k_latin_emit: the index words are loaded LATIN_EMIT_U rows ahead (the first batch before the LDS
// staging): with 2 blocks per CU the kernel is otherwise bound by waiting on them.
#ifndef LATIN_EMIT_U
#define LATIN_EMIT_U 8
#endif

// ---------------------------------------------------------------- splat
// cells of the filter-weight table by d2 (host/splat_plan.h splat_lut) that the splat kernels hold in LDS
#define SPLAT_LUT_MAX 2048

// tile pixels per lane of k_splat_col4 (its template argument NP)
#ifndef NART_SPLAT_NP
#define NART_SPLAT_NP 4
#endif
