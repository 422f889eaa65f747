// Texture.h — an image read for use as a texture (extension: the reference has no textures), host side.
// loadPPM reads binary (P6) and plain (P3) PPM files at maxval 255 into [height][width][3] floats, value / 255.f, file
// row 0 first: rt_texture's layout, in which row 0 is t = 0.  Comments (# to the end of the line) may stand anywhere
// in the header, as the format allows.  Anything else — another magic number, another maxval, a size outside
// 1..16384, a value above 255, a file that ends early — is refused with the file's name.
#pragma once

#include <cctype>
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

struct TextureImage {
  unsigned width = 0, height = 0;
  std::vector<float> texels;  // [height][width][3]

  static TextureImage loadPPM(const std::string& filename) {
    std::ifstream in(filename.c_str(), std::ios::binary);
    if (!in) throw std::runtime_error("Error loading PPM file: " + filename);
    auto bad = [&](const std::string& what) { return std::runtime_error("Error loading PPM file: " + what + " in " + filename); };
    char m0 = 0, m1 = 0;
    in.get(m0), in.get(m1);
    if (!in || m0 != 'P' || (m1 != '3' && m1 != '6')) throw bad("the magic number is neither P3 nor P6");
    const bool binary = m1 == '6';
    // a header number: white space and comments, then decimal digits (at most 6 are accepted: sizes stay far below 2^31)
    auto number = [&](const char* name) {
      int ch = in.peek();
      while (ch != EOF && (std::isspace(ch) || ch == '#')) {
        if (ch == '#')
          while (ch != EOF && ch != '\n') in.get(), ch = in.peek();
        else
          in.get(), ch = in.peek();
      }
      unsigned v = 0, digits = 0;
      while (ch != EOF && std::isdigit(ch)) {
        if (++digits > 6) throw bad(std::string(name) + " has too many digits");
        v = 10 * v + static_cast<unsigned>(ch - '0');
        in.get(), ch = in.peek();
      }
      if (digits == 0) throw bad(std::string(name) + " is missing");
      return v;
    };
    TextureImage t;
    t.width = number("the width"), t.height = number("the height");
    const unsigned maxval = number("the maximum value");
    if (t.width < 1 || t.width > 16384 || t.height < 1 || t.height > 16384) throw bad("a size outside 1..16384");
    if (maxval != 255) throw bad("a maximum value other than 255");
    const size_t n = 3 * static_cast<size_t>(t.width) * t.height;
    t.texels.resize(n);
    if (binary) {
      // exactly one white-space character separates the header from the raster
      const int sep = in.get();
      if (sep == EOF || !std::isspace(sep)) throw bad("no white space behind the header");
      std::vector<unsigned char> raw(n);
      in.read(reinterpret_cast<char*>(raw.data()), static_cast<std::streamsize>(n));
      if (static_cast<size_t>(in.gcount()) != n) throw bad("fewer bytes than the header announces");
      for (size_t i = 0; i < n; ++i) t.texels[i] = static_cast<float>(raw[i]) / 255.f;
    } else {
      for (size_t i = 0; i < n; ++i) {
        const unsigned v = number("a value");
        if (v > 255) throw bad("a value above 255");
        t.texels[i] = static_cast<float>(v) / 255.f;
      }
    }
    return t;
  }
};
