// Helper of tests/test_device_tree.py: rtaccel::float_to_half_dir (csrc/rt_accel.cpp, the host packer's outward rounding to
// binary16) on every float32 of a file.  Usage: half_dir IN OUT — IN holds raw float32 values, OUT receives two uint16 per
// value: rounded toward -inf, then toward +inf.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ray-tracing-practice_amd/csrc/rt_accel.h"

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::vector<float> x;
    float v;
    while (std::fread(&v, sizeof v, 1, in) == 1) x.push_back(v);
    std::fclose(in);
    std::vector<uint16_t> out;
    out.reserve(2 * x.size());
    for (float f : x) {
        out.push_back(rtaccel::float_to_half_dir(f, true));
        out.push_back(rtaccel::float_to_half_dir(f, false));
    }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), sizeof(uint16_t), out.size(), o) != out.size()) { std::perror(argv[2]); return 2; }
    std::fclose(o);
    std::printf("%zu values\n", x.size());
    return 0;
}
