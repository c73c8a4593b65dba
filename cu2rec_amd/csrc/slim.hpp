// SLIM (include/cu2rec_amd.h: cu2rec_slim_create): sparse item x item weights by blocked cyclic coordinate descent on EASE's
// regularised Gram matrix (slim.hip).  The model is a DeviceEase (ease.hpp), whose lists serve it unchanged.
#pragma once

#include "ease.hpp"

namespace cu2rec {

// What cu2rec_slim_create takes beside the training matrix.
struct SlimParams {
    float l1, l2;
    bool positive;
    int max_sweeps;
    float tol;
};

// the argument checks of cu2rec_slim_create that need no handle: CU2REC_EINVAL
void slim_check(const SlimParams &p);

}  // namespace cu2rec
