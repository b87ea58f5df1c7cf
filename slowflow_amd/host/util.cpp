// util.cpp -- see util.h
#include "util.h"

#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <fstream>

bool file_exists(const std::string &f) { return access(f.c_str(), F_OK) != -1; }

bool is_dir(const std::string &f) { struct stat st; return stat(f.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

void mkdirs(const std::string &path) {
    std::string cur;
    for (size_t i = 0; i <= path.size(); i++) {
        if ((i == path.size() || path[i] == '/') && !cur.empty()) mkdir(cur.c_str(), 0777);
        if (i < path.size()) cur.push_back(path[i]);
    }
}

std::string fmt1(const std::string &format, int a) { char b[1024]; snprintf(b, sizeof b, format.c_str(), a); return b; }
std::string fmt2(const std::string &format, int a, int c) { char b[1024]; snprintf(b, sizeof b, format.c_str(), a, c); return b; }

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::string sequence_frame_name(const std::string &path_format, int first, int offset, bool sintel) {
    if (!sintel) return fmt1(path_format, first + offset);
    int sintel_frame = first / 1000, hfr = offset + first % 1000;
    while (hfr < 0) { sintel_frame--; hfr += 42; }
    while (hfr > 41) { sintel_frame++; hfr -= 42; }
    return fmt2(path_format, sintel_frame, hfr);
}

std::vector<std::string> repeated(const std::string &cfg, const std::string &key) {
    std::vector<std::string> out;
    std::ifstream f(cfg.c_str(), std::ios::binary);
    std::string line;
    while (std::getline(f, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        std::vector<std::string> tok;
        size_t pos = 0;
        while (pos <= line.size()) {                                     // tabs separate, consecutive tabs collapse (parameter_list.cpp split_tabs)
            size_t next = line.find('\t', pos);
            if (next == std::string::npos) next = line.size();
            if (next > pos) tok.push_back(line.substr(pos, next - pos));
            pos = next + 1;
        }
        if (tok.size() >= 2 && tok[0] == key && tok[1][0] != '#') out.push_back(tok[1]);
    }
    return out;
}
