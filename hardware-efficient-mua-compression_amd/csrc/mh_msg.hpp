// mh_msg.hpp -- how the host-only headers report an error: the MH_* code as the return value, the text in a buffer the
// caller passes in.  Pure C++ (no HIP, no global or thread-local state): the fail() of mh_abi.hpp
// copies the text into what mh_last_error returns and stays the only writer of that; tests/planner_check.cpp prints it.
#pragma once
#include <cstdarg>
#include <cstdio>

namespace mh {

struct Msg {
    char text[512];  // (the size of the libraries' last-error buffers)

    Msg() { text[0] = 0; }
    // formats the message and returns `code`:  return m.set(MH_ERR_ARG, "C=%u", C);
    __attribute__((format(printf, 3, 4))) int set(int code, const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return code;
    }
};

}  // namespace mh
