// The preamble every host-sanitizer driver (tests/host_san*/driver.cpp, built and run by tests/host_san_build.py) shares: the
// C ABI, the HIP stand-in of this directory, and the checks.  The macros are for functions that return int and report a
// failure as `return 1` with file and line on stderr; OK and REFUSED read the handle `h` of the scope they stand in.
//   CHECK(cond)                 cond holds
//   OK(call)                    call returns TVC_OK
//   REFUSED(call, code, word)   call returns `code` and leaves a tvc_last_error that contains `word`
//   dev(bytes)                  a "device" block of exactly that size (16 bytes for 0), never NULL
// A driver that wants a line of its own ahead of every OK call defines DRIVER_BEFORE_OK(text) before it includes this file
// (text is the call as written).
#pragma once
#include "../../include/tvc.h"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#ifndef DRIVER_BEFORE_OK
#define DRIVER_BEFORE_OK(text) ((void)0)
#endif

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)
#define OK(call)                                                                                           \
    do {                                                                                                   \
        DRIVER_BEFORE_OK(#call);                                                                           \
        int rc__ = (call);                                                                                 \
        if (rc__ != TVC_OK) { fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc__, tvc_last_error(h)); return 1; } \
    } while (0)
#define REFUSED(call, code, word)                                                                \
    do {                                                                                         \
        CHECK((call) == (code));                                                                 \
        CHECK(strstr(tvc_last_error(h), word) != nullptr);                                       \
    } while (0)

static void* dev(size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) abort(); return p; }
