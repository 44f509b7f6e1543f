// lightglue_amd — the library-wide error state and version string of the C ABI (include/lightglue_amd.h): every entry point
// (matcher engine, SuperPoint, ALIKED, preprocessor) reports through lg::set_error.
#include <string>

#include "../../include/lightglue_amd.h"
#include "lg_kernels.h"

namespace {
thread_local std::string g_err = "";
}  // namespace

namespace lg {
int set_error(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace lg

extern "C" {

const char* lg_last_error(void) { return g_err.c_str(); }
const char* lg_version(void) { return "lightglue_amd 0.6 (gfx950)"; }

}  // extern "C"
