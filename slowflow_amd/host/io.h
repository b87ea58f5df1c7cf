// io.h -- the file formats either side of the path, without third-party image libraries:
//   .flo  Middlebury flow (float 202021.25, int w, int h, interleaved u,v rows) -- io.c:53-101 of the reference
//   .ppm / .pgm  binary P6 / P5, 8 or 16 bit (big-endian samples), .pfm (Pf / PF, float) and .png (png.h)
//   .pgm / .pbm  binary P5 (maxval 255) / P4 as 8-bit grey planes, for the masks and maps of the accumulate program
#ifndef SLOWFLOW_AMD_HOST_IO_H
#define SLOWFLOW_AMD_HOST_IO_H

#include <string>
#include <vector>

#include "image.h"

int writeFlowFile(const char *filename, const image_t *flowx, const image_t *flowy);   /* 0 on success */
image_t **readFlowFile(const char *filename);                                           /* [0]=u, [1]=v; NULL on failure */
/* loads a frame as 3 float planes (grey images are replicated); *maxval = 255 / 65535 / 1 (pfm). NULL on failure */
color_image_t *color_image_load(const char *filename, int *maxval);
/* binary P5, 8 bit: value = clamp(round(scale * (v + offset)), 0, 255); 0 on success */
int writePGM(const char *filename, const image_t *img, float offset, float scale);
/* binary PGM (P5, maxval 255) or PBM (P4: bit 1 = black = 0, bit 0 = white = 255, as OpenCV reads it) -> w x h 8-bit grey values; false on failure */
bool read_pnm8(const std::string &file, int &w, int &h, std::vector<unsigned char> &px);
/* binary P5, maxval 255, of w x h 8-bit values whose rows are `stride` bytes apart */
bool write_pgm8(const std::string &file, int w, int h, const unsigned char *px, int stride);
/* little-endian PFM (Pf, scale -1), rows bottom to top as color_image_load reads them; px: w x h floats, rows w apart */
bool write_pfm(const std::string &file, int w, int h, const float *px);

#endif
