// util.h -- small helpers the host programs (slow_flow, adaptiveFR, accumulate) share: files and folders, printf-style names, the sequences' frame
// names and the cfg keys the reference collects rather than keeps one value of.
#ifndef SLOWFLOW_AMD_HOST_UTIL_H
#define SLOWFLOW_AMD_HOST_UTIL_H

#include <string>
#include <vector>

bool file_exists(const std::string &f);
bool is_dir(const std::string &f);
/* mkdir -p: every folder along `path` ('/'-separated; the last component is made as well) */
void mkdirs(const std::string &path);
/* snprintf(format, a) / snprintf(format, a, b) into at most 1023 characters */
std::string fmt1(const std::string &format, int a);
std::string fmt2(const std::string &format, int a, int b);
/* seconds on the steady clock */
double now_s();
/* the file of frame first + offset of a sequence (path_format: a printf pattern).  Sintel numbers first as scene * 1000 + frame and its
 * scenes hold 42 frames: the name is path_format % (scene, frame) with the frame wrapped into 0..41 */
std::string sequence_frame_name(const std::string &path_format, int first, int offset, bool sintel);
/* every value of `key` in a cfg, in file order (utils/parameter_list.cpp:113-130): lines "key<TAB>value", runs of tabs collapse, CR / LF
 * stripped, values starting with '#' skipped */
std::vector<std::string> repeated(const std::string &cfg, const std::string &key);

#endif
