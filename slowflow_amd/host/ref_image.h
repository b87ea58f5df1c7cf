// ref_image.h -- dense_tracking's reduced reference image on the host (dense_tracking.cpp:931-936): frame 0 as 8 bits, OpenCV's 8-bit GaussianBlur and
// resize(INTER_LINEAR) to the accumulation grid, in the integer arithmetic INTEGRATION.md 4c' defines (csrc/ref_image.h: taps, tie rule, sizes; OpenCV is
// not in this tree, so the stage is parity-unpinned against it).  The plain C++ form the kernel of csrc/ref_image.hip is tested against.
#ifndef SLOWFLOW_AMD_HOST_REF_IMAGE_H
#define SLOWFLOW_AMD_HOST_REF_IMAGE_H

#include "image.h"

// rgb as read (before normalize), norm 1/255 for 16-bit input and 1 otherwise, skip = acc_skip_pixel -> the 8-bit image at the grid's size, its values
// 0 .. 255 as floats (what rgb_to_lab takes and the edge detector's PNG holds).  Null where skip is not served or OpenCV's resize would give another size
// than the accumulation grid.  The caller deletes the image.
color_image_t *reference_rgb8(const color_image_t *rgb, float norm, int skip);

#endif
