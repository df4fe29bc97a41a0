// The photometric stage (include/ccal.h, "the photometric stage"; ccal_kernels_photo.hip) as the renderer's host code sees it:
//   PhotoTables    what the kernel takes by value: the radius, the taps and the noise table, made on the host
//   photo_check    the check of the options; fills the tables
//   photo_enqueue  one launch on a stream over n_img images whose first has the noise stream `stream0` (seed + first_index + its
//                  index in the call); the caller has checked the image arguments
// Host only.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/ccal.h"

namespace ccal {

struct PhotoTables {
    int32_t radius, reserved_;
    double taps[CCAL_PHOTO_MAX_RADIUS + 1];
    double sigma[256];
};

// nullptr and the tables filled, or the message of the first option out of range (photo != NULL)
const char* photo_check(const ccal_photo_opts* photo, PhotoTables* tables);

hipError_t photo_enqueue(hipStream_t st, const PhotoTables& tables, const ccal_photo_opts& photo, int src_dtype, int dst_dtype, int width,
                         int height, int n_img, uint64_t stream0, const void* src, void* dst);

}  // namespace ccal
