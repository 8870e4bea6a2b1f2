// mh_abi.hpp -- how every entry point of every library ends: the thread's last error text, fail() that writes it and
// launched() that asks the runtime what the launches left behind.  Included once by each .hip, with internal linkage:
// every shared object has its own buffer and exports none of this (its mhX_last_error returns g_err).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "mh_msg.hpp"
#include "muahuff.h"

namespace {

thread_local char g_err[sizeof(mh::Msg::text)] = "";

[[maybe_unused]] int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// what a host-only header reported (mh_msg.hpp)
[[maybe_unused]] int fail(int code, const mh::Msg &m) { return fail(code, "%s", m.text); }

// how an entry point that launches ends: MH_OK, or what its launches left behind.  `fn` names the entry point.
[[maybe_unused]] int launched(const char *fn)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MH_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return MH_OK;
}

// fn(std::integral_constant<int, K>) for K = k, where a kernel is instantiated per k = 1..8; k has passed its check, and
// anything else takes 8
template <class Fn>
void dispatch_k(uint32_t k, Fn &&fn)
{
    switch (k) {
    case 1: fn(std::integral_constant<int, 1>()); break;
    case 2: fn(std::integral_constant<int, 2>()); break;
    case 3: fn(std::integral_constant<int, 3>()); break;
    case 4: fn(std::integral_constant<int, 4>()); break;
    case 5: fn(std::integral_constant<int, 5>()); break;
    case 6: fn(std::integral_constant<int, 6>()); break;
    case 7: fn(std::integral_constant<int, 7>()); break;
    default: fn(std::integral_constant<int, 8>()); break;
    }
}

}  // namespace
