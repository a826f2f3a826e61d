// Shared by the TORCH_LIBRARY fragments in this directory.
#pragma once

#include <c10/hip/HIPStream.h>

namespace {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

}  // namespace
