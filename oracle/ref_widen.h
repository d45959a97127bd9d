/*
 * ref_widen.h -- force-included (-include) in front of every reference file and
 * of ref_shim.cpp when oracle/Makefile builds _ref/libgg_ref.so.
 *
 * TEST INFRASTRUCTURE ONLY.  The reference computes in float, the oracle in
 * double.  Redefining `float` on the command line (-Dfloat=double) would also
 * rewrite the C and C++ library headers, where float and double overloads then
 * collide.  So every system header the reference files reach is included here
 * first, with `float` untouched; their include guards make the later #include
 * lines no-ops, and only the reference's own text (and its own headers) is
 * read with float = double.  src/defs.h's eps becomes the double 1e-9 that
 * oracle.c's is_zero uses.
 */
#ifndef GG_REF_WIDEN_H_
#define GG_REF_WIDEN_H_

#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#define float double

#endif
