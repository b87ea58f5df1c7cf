// Host side of tests/test_track_fill.py: the Lab image the accumulate program uploads with a start_jet, from the host's own rgb_to_lab (host/epic.cpp).
//   lab_tool <rgb.bin> <w> <h> <lab.bin>
//       rgb.bin: 3 planes of h * stride floats holding 8-bit values (stride = color_image_new's); lab.bin: the same layout.  No GPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "epic.h"

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: lab_tool rgb.bin w h lab.bin\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    color_image_t *rgb = color_image_new(w, h);
    const std::streamsize bytes = (std::streamsize)((size_t)3 * rgb->stride * h * sizeof(float));
    std::ifstream in(argv[1], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(rgb->c1), bytes)) { fprintf(stderr, "%s: not 3 x %d x %d floats\n", argv[1], h, rgb->stride); return 2; }
    color_image_t *lab = rgb_to_lab(rgb);
    std::ofstream out(argv[4], std::ios::binary);
    out.write(reinterpret_cast<const char *>(lab->c1), bytes);
    color_image_delete(rgb);
    color_image_delete(lab);
    return out.good() ? 0 : 1;
}
