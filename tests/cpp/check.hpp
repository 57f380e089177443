/* check.hpp — how every program under tests/cpp ends on an error: CHECK for
 * a HIP call, FAIL for a verdict of its own. Both print to stdout, which the
 * Python tests show, and exit with status 1. */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(c)                                                      \
  do {                                                                \
    hipError_t e = (c);                                               \
    if (e != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    exit(1);             \
  } while (0)
