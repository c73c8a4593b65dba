// rocPRIM's two-call form (als.hip: the item-major view's sort; bpr.hip: the rows' items and the negatives' regrouping): a call with
// a null temporary only reports the bytes it needs, the same call with that many does the work.
#pragma once

#include <cstddef>

#include "hip_check.hpp"

namespace cu2rec {

// call(temp, bytes): the rocPRIM call with all but its first two arguments bound.  temp grows to what the call asks for and 16 bytes
// of slack, and never shrinks: a cached buffer or a fresh local one, as the caller has it
template <class Call>
void with_rocprim_temp(DeviceBuffer<unsigned char> &temp, Call &&call) {
    size_t bytes = 0;
    CU2REC_HIP(call(nullptr, bytes));
    if (temp.count < bytes + 16) temp.allocate(bytes + 16);
    CU2REC_HIP(call(temp.ptr, bytes));
}

}  // namespace cu2rec
