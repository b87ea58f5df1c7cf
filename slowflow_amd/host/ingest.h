// ingest.h -- what the driver does to a frame between the file and the path (slow_flow.cpp:447-600), without OpenCV:
// Bayer demosaicing (the reference's own bilinear / green-ratio routine), raw channel weighting, cropping, and the
// anti-aliased rescaling (cv::GaussianBlur + cv::resize semantics, run through the C-ABI's pyramid operators).
#ifndef SLOWFLOW_AMD_HOST_INGEST_H
#define SLOWFLOW_AMD_HOST_INGEST_H

#include <string>
#include <vector>

#include "../../include/slowflow_amd.h"
#include "image.h"

/* utils.cpp:1336-1374: per-pixel data-term weights of the three channels for a Bayer mosaic whose first red pixel sits at
 * (red_x, red_y); the measured colour of a pixel gets `weight` (clamped to [0,3]), the two interpolated ones (3-weight)/2 */
void rawWeighting(color_image_t *weights, int red_x, int red_y, float weight);
/* utils.cpp:1241-1334 (bayer2rgbGR): green by 4-neighbour averaging, red / blue through the local green ratio; mirrored
 * borders.  src: the mosaic (1 plane), dst: R, G, B planes */
void bayer2rgbGR(const image_t *src, color_image_t *dst, int red_x, int red_y);
/* raw_demosaicing 2 (slow_flow.cpp:502-520): the mosaic is converted to 8 bit with saturation (Mat::convertTo(CV_8UC1): round half to even, clamp)
 * and demosaiced as cv::cvtColor(CV_Bayer*2RGB) does on 8-bit data: at a red / blue site green = (4 neighbours + 2) >> 2 and the opposite colour =
 * (4 diagonals + 2) >> 2, at a green site each colour = (its 2 neighbours + 1) >> 1; the outermost rows and columns repeat their inner neighbours.
 * OpenCV is not in this image: the arithmetic is restated from its documented bilinear Bayer conversion, parity unpinned.  dst: R, G, B planes, 0..255 */
void bayer2rgb_cv8u(const image_t *src, color_image_t *dst, int red_x, int red_y);
/* a frame file decoded (color_image_load; *maxval as it sets it) and, where `raw`, demosaiced from its grey mosaic whose first red pixel sits at
 * (red_x, red_y): demosaicing 2 is bayer2rgb_cv8u, any other value bayer2rgbGR.  NULL on failure, with the message in *error.  No shared
 * state and no printing of its own: the driver's decoding tasks call it in parallel */
color_image_t *load_frame(const std::string &file, bool raw, int demosaicing, int red_x, int red_y, int *maxval, std::string *error);
/* gpu_ingest 1: a frame file decoded to its one-channel mosaic only (the first plane color_image_load returns, what load_frame demosaics), rows packed.
 * Samples of an integer format travel as uint8 / uint16 (sfa_dev_dtype; (float) of them is the plane's value exactly), anything else as fp32 */
struct Mosaic {
    int width = 0, height = 0, dtype = SFA_DEV_F32, maxval = 255;
    std::vector<unsigned char> data;
};
bool load_mosaic(const std::string &file, Mosaic *out, std::string *error);
/* img.rowRange / colRange of slow_flow.cpp:543-546; returns a new image (caller frees) */
color_image_t *color_image_crop(const color_image_t *img, int center_x, int center_y, int extent_x, int extent_y);
/* slow_flow.cpp:550-553: GaussianBlur(sigma = 1/sqrt(2*scale), BORDER_REPLICATE) then resize(Size(0,0), scale, scale,
 * INTER_LINEAR); returns a new image of cvRound(w*scale) x cvRound(h*scale) or NULL (see sfa_last_error) */
color_image_t *color_image_rescale(sfa_ctx *ctx, const color_image_t *img, float scale);

#endif
