// em2_entry.h -- what a C entry point of include/em2_lsh.h needs around its one em2::run... call: the error reporters that
// set em2_last_error (the thread-local slot itself is em2_capi.hip's), the device check, and the two macros that turn a failed
// HIP call into EM2_ERROR_HIP.  Every .hip file that defines extern "C" entries includes it and says
// `using namespace em2::entry;`.
#ifndef EM2_ENTRY_H
#define EM2_ENTRY_H

#include "../../include/em2_lsh.h"

#include "em2_hip_util.h"

#include <string>

// Defined in em2_capi.hip, next to the slot.
extern "C" void em2_internal_set_last_error(const char* message);

namespace em2 {
namespace entry {

inline int fail(int code, const std::string& message)
{
    em2_internal_set_last_error(message.c_str());
    return code;
}

// An argument error under the caller's name: what UploadedCsr::check or em2::inputErrorText says.
inline int failArgument(const char* who, const char* text) { return fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": " + text); }

inline int failNull(const char* who) { return failArgument(who, "null pointer"); }

inline int failNoDevice(const char* who)
{
    return fail(EM2_ERROR_NO_DEVICE, std::string(who) + ": no HIP device is visible (this library has no CPU path)");
}

inline bool haveDevice()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

}  // namespace entry
}  // namespace em2

// Returns EM2_ERROR_HIP from the enclosing entry point when the call fails, as "<who>: <hipGetErrorString>" ...
#define EM2_HIP_FOR(who, call)                                                                                       \
    do {                                                                                                             \
        const hipError_t em2HipError_ = (call);                                                                      \
        if (em2HipError_ != hipSuccess) return ::em2::entry::fail(EM2_ERROR_HIP, std::string(who) + ": " + hipGetErrorString(em2HipError_)); \
    } while (0)

// ... or as "<text of the call>: <hipGetErrorString>".
#define EM2_HIP(call) EM2_HIP_FOR(#call, call)

#endif
