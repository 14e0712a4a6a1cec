// expect.h — the check of the host sanitizer programs (host/asan_*.cpp): EXPECT(c) prints the failed condition with its
// place and counts it; main returns 1 if `failures` is not 0.  One program, one translation unit.
#pragma once
#include <cstdio>

static int failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                \
        }                                                              \
    } while (0)
