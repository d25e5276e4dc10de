#include "texture_io.h"

#include "jpeg_decoder.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

namespace rtp {

void ldr_to_linear_rgba(const unsigned char *px, int width, int height, int channels, TextureImage &out) {
    out.width = width;
    out.height = height;
    out.rgba.resize(static_cast<size_t>(width) * height * 4);
    // 256-entry table of pow(c/255.0f, 2.2f) evaluated like stb does: float divide, double pow.
    float lut[256];
    for (int c = 0; c < 256; ++c) lut[c] = static_cast<float>(pow(c / 255.0f, 2.2f) * 1.0f);
    for (size_t i = 0; i < static_cast<size_t>(width) * height; ++i) {
        for (int k = 0; k < 3; ++k) out.rgba[i * 4 + k] = lut[px[i * channels + (channels >= 3 ? k : 0)]];
        out.rgba[i * 4 + 3] = channels == 4 ? px[i * 4 + 3] / 255.0f : 1.0f;
    }
}

namespace {
bool read_token(std::istream &in, std::string &tok) {
    tok.clear();
    int c;
    while ((c = in.get()) != EOF) {
        if (c == '#') { while ((c = in.get()) != EOF && c != '\n') {} continue; }
        if (!isspace(c)) { tok.push_back(static_cast<char>(c)); break; }
    }
    while ((c = in.peek()) != EOF && !isspace(c)) tok.push_back(static_cast<char>(in.get()));
    return !tok.empty();
}
}  // namespace

bool load_texture(const std::string &path, TextureImage &out) {
    {   // JPEG (SOI marker FF D8): the reference's floor textures are JPEGs
        std::ifstream probe(path, std::ios::binary);
        unsigned char magic[2] = {0, 0};
        probe.read(reinterpret_cast<char *>(magic), 2);
        if (probe.gcount() == 2 && magic[0] == 0xFF && magic[1] == 0xD8) {
            int w = 0, h = 0;
            std::vector<uint8_t> rgb;
            if (!decode_jpeg_rgb8(path, w, h, rgb)) {
                std::cerr << "Failed to load texture: " << path << std::endl;
                return false;
            }
            ldr_to_linear_rgba(rgb.data(), w, h, 3, out);
            return true;
        }
    }
    std::ifstream in(path, std::ios::binary);
    std::string magic, tw, th, tmax;
    if (!in || !read_token(in, magic) || (magic != "P6" && magic != "PF") || !read_token(in, tw) ||
        !read_token(in, th) || !read_token(in, tmax)) {
        std::cerr << "Failed to load texture: " << path << std::endl;
        return false;
    }
    in.get();  // single whitespace after the header
    const int w = atoi(tw.c_str()), h = atoi(th.c_str());
    // same caps as the JPEG path: a hostile header must not size a multi-gigabyte allocation
    if (w <= 0 || h <= 0 || w > 16384 || h > 16384 || static_cast<long long>(w) * h > (1ll << 26)) {
        std::cerr << "Failed to load texture: " << path << std::endl;
        return false;
    }
    const size_t n = static_cast<size_t>(w) * h;
    if (magic == "P6") {
        std::vector<unsigned char> buf(n * 3);
        in.read(reinterpret_cast<char *>(buf.data()), static_cast<std::streamsize>(buf.size()));
        if (in.gcount() != static_cast<std::streamsize>(buf.size()) || atoi(tmax.c_str()) != 255) {
            std::cerr << "Failed to load texture: " << path << std::endl;
            return false;
        }
        ldr_to_linear_rgba(buf.data(), w, h, 3, out);
        return true;
    }
    // PF: little-endian float RGB when the scale token is negative; rows bottom to top.
    std::vector<float> buf(n * 3);
    in.read(reinterpret_cast<char *>(buf.data()), static_cast<std::streamsize>(buf.size() * 4));
    if (in.gcount() != static_cast<std::streamsize>(buf.size() * 4) || atof(tmax.c_str()) >= 0) {
        std::cerr << "Failed to load texture: " << path << std::endl;
        return false;
    }
    out.width = w;
    out.height = h;
    out.rgba.resize(n * 4);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const float *s = &buf[(static_cast<size_t>(h - 1 - y) * w + x) * 3];
            float *d = &out.rgba[(static_cast<size_t>(y) * w + x) * 4];
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = 1.0f;
        }
    return true;
}

namespace {
bool hdr_size_ok(long long w, long long h) { return w > 0 && h > 0 && w <= 16384 && h <= 16384 && w * h <= (1ll << 26); }

bool load_pfm(std::istream &in, HdrImage &out, std::string &error) {
    std::string magic, tw, th, tscale;
    if (!read_token(in, magic) || magic != "PF" || !read_token(in, tw) || !read_token(in, th) || !read_token(in, tscale)) {
        error = "malformed PFM header";
        return false;
    }
    in.get();  // single whitespace after the header
    const long long w = atoll(tw.c_str()), h = atoll(th.c_str());
    const double scale = atof(tscale.c_str());
    if (!hdr_size_ok(w, h) || scale == 0.0) {
        error = "PFM size or scale out of range";
        return false;
    }
    const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
    std::vector<unsigned char> buf(n * 12);
    in.read(reinterpret_cast<char *>(buf.data()), static_cast<std::streamsize>(buf.size()));
    if (in.gcount() != static_cast<std::streamsize>(buf.size())) {
        error = "truncated PFM";
        return false;
    }
    const bool big = scale > 0.0;          // a negative scale token: little-endian floats
    out.width = static_cast<int>(w);
    out.height = static_cast<int>(h);
    out.rgb.resize(n * 3);
    for (long long y = 0; y < h; ++y)
        for (long long k = 0; k < w * 3; ++k) {
            const unsigned char *b = &buf[(static_cast<size_t>(h - 1 - y) * w * 3 + k) * 4];
            const uint32_t bits = big ? (uint32_t(b[0]) << 24 | uint32_t(b[1]) << 16 | uint32_t(b[2]) << 8 | uint32_t(b[3]))
                                      : (uint32_t(b[3]) << 24 | uint32_t(b[2]) << 16 | uint32_t(b[1]) << 8 | uint32_t(b[0]));
            float f;
            memcpy(&f, &bits, 4);
            out.rgb[static_cast<size_t>(y) * w * 3 + k] = f;
        }
    return true;
}

bool load_rgbe(std::istream &in, HdrImage &out, std::string &error) {
    std::string line;
    if (!std::getline(in, line) || line.compare(0, 10, "#?RADIANCE") != 0) {
        error = "not a Radiance file";
        return false;
    }
    bool format_ok = true;
    while (std::getline(in, line) && !line.empty() && line != "\r")
        if (line.compare(0, 7, "FORMAT=") == 0 && line.compare(7, 15, "32-bit_rle_rgbe") != 0) format_ok = false;
    long long w = 0, h = 0;
    char sy = 0, sx = 0, ay = 0, ax = 0;
    if (!in || !format_ok || !std::getline(in, line) || sscanf(line.c_str(), "%c%c %lld %c%c %lld", &sy, &ay, &h, &sx, &ax, &w) != 6 || sy != '-' ||
        ay != 'Y' || sx != '+' || ax != 'X' || !hdr_size_ok(w, h)) {
        error = "malformed Radiance header (FORMAT=32-bit_rle_rgbe and -Y h +X w are read)";
        return false;
    }
    out.width = static_cast<int>(w);
    out.height = static_cast<int>(h);
    out.rgb.resize(static_cast<size_t>(w) * h * 3);
    std::vector<unsigned char> row(static_cast<size_t>(w) * 4);
    for (long long y = 0; y < h; ++y) {
        unsigned char head[4];
        in.read(reinterpret_cast<char *>(head), 4);
        if (in.gcount() != 4) { error = "truncated Radiance scanline"; return false; }
        if (w >= 8 && w <= 0x7fff && head[0] == 2 && head[1] == 2 && (head[2] & 0x80) == 0) {       // new-style run-length encoding
            if ((static_cast<long long>(head[2]) << 8 | head[3]) != w) { error = "Radiance scanline of the wrong width"; return false; }
            for (int c = 0; c < 4; ++c) {
                long long x = 0;
                while (x < w) {
                    int count = in.get();
                    if (count == EOF) { error = "truncated Radiance scanline"; return false; }
                    if (count > 128) {
                        count -= 128;
                        const int value = in.get();
                        if (value == EOF || x + count > w) { error = "malformed Radiance run"; return false; }
                        for (int k = 0; k < count; ++k) row[static_cast<size_t>(x++) * 4 + c] = static_cast<unsigned char>(value);
                    } else {
                        if (count == 0 || x + count > w) { error = "malformed Radiance run"; return false; }
                        for (int k = 0; k < count; ++k) {
                            const int value = in.get();
                            if (value == EOF) { error = "truncated Radiance scanline"; return false; }
                            row[static_cast<size_t>(x++) * 4 + c] = static_cast<unsigned char>(value);
                        }
                    }
                }
            }
        } else {                                                                                        // flat: w pixels of four bytes
            memcpy(row.data(), head, 4);
            in.read(reinterpret_cast<char *>(row.data() + 4), static_cast<std::streamsize>((w - 1) * 4));
            if (in.gcount() != static_cast<std::streamsize>((w - 1) * 4)) { error = "truncated Radiance scanline"; return false; }
        }
        for (long long x = 0; x < w; ++x) {
            const unsigned char *p = &row[static_cast<size_t>(x) * 4];
            const float f = p[3] ? std::ldexp(1.0f, static_cast<int>(p[3]) - 136) : 0.0f;
            float *d = &out.rgb[(static_cast<size_t>(y) * w + x) * 3];
            d[0] = p[0] * f; d[1] = p[1] * f; d[2] = p[2] * f;
        }
    }
    return true;
}
}  // namespace

bool load_hdr_image(const std::string &path, HdrImage &out, std::string &error) {
    std::ifstream in(path, std::ios::binary);
    char magic[2] = {0, 0};
    if (!in || !in.read(magic, 2)) {
        error = "cannot read " + path;
        return false;
    }
    in.seekg(0);
    bool ok = false;
    if (magic[0] == 'P' && magic[1] == 'F') ok = load_pfm(in, out, error);
    else if (magic[0] == '#' && magic[1] == '?') ok = load_rgbe(in, out, error);
    else error = "neither a PFM (PF) nor a Radiance (#?RADIANCE) file";
    if (!ok) error = path + ": " + error;
    return ok;
}

void make_checker_texture(int size, TextureImage &out) {
    std::vector<unsigned char> px(static_cast<size_t>(size) * size * 3);
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x) {
            const bool dark = (((x * 16) / size) + ((y * 16) / size)) & 1;
            unsigned char *p = &px[(static_cast<size_t>(y) * size + x) * 3];
            p[0] = static_cast<unsigned char>(dark ? 60 : 200 + (x * 55) / size);
            p[1] = static_cast<unsigned char>(dark ? 70 : 190);
            p[2] = static_cast<unsigned char>(dark ? 90 + (y * 100) / size : 170);
        }
    ldr_to_linear_rgba(px.data(), size, size, 3, out);
}

}  // namespace rtp
