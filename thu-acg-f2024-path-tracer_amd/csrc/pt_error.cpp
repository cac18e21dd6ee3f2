// The error channel of the C ABI and the experiment switches' gate (host-only). See pt_scene.h.
#include <cstdlib>

#include "pt_scene.h"

namespace pt {
static thread_local std::string g_error;
int set_error(const std::string& msg) {
    g_error = msg;
    return -1;
}
const char* last_error() { return g_error.c_str(); }
const char* exp_env(const char* name) {
    const char* on = getenv("PT_EXPERIMENT");
    return (on && on[0] == '1') ? getenv(name) : nullptr;
}
}  // namespace pt

extern "C" const char* pt_last_error(void) { return pt::last_error(); }
extern "C" int pt_set_error_message(const char* msg) { return pt::set_error(msg); }
