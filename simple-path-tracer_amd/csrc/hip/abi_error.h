// How the code behind the C ABI refuses a call: fail() throws, the entry point (guarded, spt_hip.hip) turns the exception into the
// call's status and the message of spt_last_error.  Shared by the runtime side (spt_hip.hip) and the scene builder (scene_build.h).
#pragma once
#include <string>

#include "../../../include/spt_abi.h"

struct AbiError {
    spt_status code;
    std::string msg;
};
[[noreturn]] inline void fail(spt_status code, const std::string& msg) { throw AbiError{code, msg}; }
