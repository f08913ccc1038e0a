// params_tool.cpp -- halo2's ParamsKZG::{read_custom, write_custom, downsize} and a consistency check of a params file, from plain C++ over
// the C ABI (include/pz.h: pz_params_*).  No torch, no HIP call of its own, no Python.  Every point is decoded and checked on the device.
//
// usage: params_tool check <file>
//        params_tool convert <in> <processed | raw> <out>
//        params_tool downsize <in> <k> <out>
//   The input's format (SerdeFormat::Processed: 32-byte G1 and 64-byte G2 points; RawBytes: the ABI's words) is taken from its size, which is
//   unambiguous for the k in its header.  convert and downsize refuse a file with a point off its curve (pz_params_decode, as halo2's
//   read_custom does); downsize writes the input's format.
//   check decodes a raw file WITHOUT the per-point refusal, so that pz_params_check names what is wrong with it.
// stdout (check): one JSON line {"k", "format", "failed": [names], "skipped": [names]}; the names are BAD_G1, BAD_G2, BAD_G0, BAD_POWERS,
//   BAD_LAGRANGE (include/pz.h).  An empty "failed" says the four sections form one SRS for SOME s -- not that nobody knows s.
// Exit 0 ok; 1 check found a failure; 2 malformed arguments or files, a refused point, or a library error.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pz.h"

namespace {

int fail(const char* what) {
    fprintf(stderr, "params_tool: %s\n", what);
    return 2;
}

struct Mapped {   // a file mapped read-only (a k = 26 file is 8.6 GB: not read into memory)
    const uint8_t* p = nullptr;
    size_t len = 0;
    bool open(const char* path) {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) {
            close(fd);
            return false;
        }
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return false;
        p = (const uint8_t*)m;
        len = (size_t)st.st_size;
        return true;
    }
    ~Mapped() {
        if (p) munmap((void*)p, len);
    }
};

// the format of a file from its size and header; -1 if neither fits
int format_of(const Mapped& f, uint32_t* k) {
    if (f.len < 4) return -1;
    memcpy(k, f.p, 4);
    for (int fmt : {PZ_SERDE_PROCESSED, PZ_SERDE_RAW}) {
        size_t want = 0;
        if (pz_params_file_bytes(*k, fmt, &want) == PZ_OK && want == f.len) return fmt;
    }
    return -1;
}

bool parse_format(const char* s, int* fmt) {
    const std::string v = s;
    if (v == "processed" || v == "0") *fmt = PZ_SERDE_PROCESSED;
    else if (v == "raw" || v == "1") *fmt = PZ_SERDE_RAW;
    else return false;
    return true;
}

const char* format_name(int fmt) { return fmt == PZ_SERDE_PROCESSED ? "processed" : "raw"; }

std::string names(uint32_t bits) {
    static const char* const NAMES[5] = {"BAD_G1", "BAD_G2", "BAD_G0", "BAD_POWERS", "BAD_LAGRANGE"};
    std::string out = "[";
    for (int i = 0; i < 5; ++i)
        if (bits >> i & 1) out += std::string(out.size() > 1 ? ", " : "") + "\"" + NAMES[i] + "\"";
    return out + "]";
}

int write_params(const pz_params* params, uint32_t k, int fmt, const char* path) {
    size_t bytes = 0;
    if (pz_params_file_bytes(k, fmt, &bytes) != PZ_OK) return fail("pz_params_file_bytes");
    std::vector<uint8_t> out(bytes);
    const int rc = pz_params_encode(params, fmt, out.data(), out.size());
    if (rc != PZ_OK) {
        fprintf(stderr, "params_tool: pz_params_encode: %s\n", pz_strerror(rc));
        return 2;
    }
    FILE* f = fopen(path, "wb");
    if (!f) return fail("cannot write the output file");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) return fail("cannot write the output file");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    static const char* const USAGE = "usage: params_tool check <file> | convert <in> <processed | raw> <out> | downsize <in> <k> <out>";
    if (argc < 3) return fail(USAGE);
    const std::string cmd = argv[1];
    int out_fmt = -1;
    uint64_t k_new = 0;
    if (cmd == "check") {
        if (argc != 3) return fail(USAGE);
    } else if (cmd == "convert") {
        if (argc != 5) return fail(USAGE);
        if (!parse_format(argv[3], &out_fmt)) return fail("format: processed | raw");
    } else if (cmd == "downsize") {
        if (argc != 5) return fail(USAGE);
        char* end = nullptr;
        k_new = strtoull(argv[3], &end, 10);
        if (!*argv[3] || *end || k_new < 1 || k_new > 28) return fail("k: a number in 1..28");
    } else {
        return fail(USAGE);
    }
    Mapped in;
    if (!in.open(argv[2])) return fail("cannot read the params file");
    uint32_t k = 0;
    const int fmt = format_of(in, &k);
    if (fmt < 0) return fail("params file: its size fits neither format for the k in its header");
    if (cmd == "downsize" && k_new > k) return fail("downsize: k exceeds the file's");

    pz_ctx* ctx = nullptr;
    const int dev = 0;
    if (pz_init(1, &dev, &ctx) != PZ_OK) return fail("pz_init");
    pz_params *params = nullptr, *small = nullptr;
    uint64_t n_bad = 0;
    const int read_fmt = cmd == "check" && fmt == PZ_SERDE_RAW ? PZ_SERDE_RAW_UNCHECKED : fmt;
    int rc = pz_params_decode(ctx, in.p, in.len, read_fmt, &params, &n_bad);
    int code = 0;
    if (rc != PZ_OK) {
        fprintf(stderr, "params_tool: pz_params_decode: %s (%llu points refused)\n", pz_strerror(rc), (unsigned long long)n_bad);
        code = 2;
    } else if (cmd == "check") {
        uint32_t failed = 0, skipped = 0;
        rc = pz_params_check(params, &failed, &skipped);
        if (rc != PZ_OK) {
            fprintf(stderr, "params_tool: pz_params_check: %s\n", pz_strerror(rc));
            code = 2;
        } else {
            printf("{\"k\": %u, \"format\": \"%s\", \"failed\": %s, \"skipped\": %s}\n", k, format_name(fmt), names(failed).c_str(),
                   names(skipped).c_str());
            code = failed ? 1 : 0;
        }
    } else if (cmd == "convert") {
        code = write_params(params, k, out_fmt, argv[4]);
    } else {
        rc = pz_params_downsize(params, (uint32_t)k_new, &small);
        if (rc != PZ_OK) {
            fprintf(stderr, "params_tool: pz_params_downsize: %s\n", pz_strerror(rc));
            code = 2;
        } else {
            code = write_params(small, (uint32_t)k_new, fmt, argv[4]);
        }
    }
    pz_params_free(small);
    pz_params_free(params);
    pz_free(ctx);
    return code;
}
