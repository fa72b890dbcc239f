// What every *_harness.cpp here shares: the failure counter, CHECK and the closing line.  A harness is
// one translation unit, so the counter is a static of that unit.
#pragma once

#include <cstdio>

static int g_bad = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);    \
            ++g_bad;                                              \
        }                                                         \
    } while (0)

// The last line of main: "<name> harness ok", which the tests look for, or the count of failed
// checks; the value is the exit status.
static inline int harness_done(const char *name)
{
    if (g_bad)
        std::printf("%s harness: %d FAILED\n", name, g_bad);
    else
        std::printf("%s harness ok\n", name);
    return g_bad ? 1 : 0;
}
