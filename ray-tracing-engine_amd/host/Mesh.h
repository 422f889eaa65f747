// Mesh.h — indexed triangle mesh container + OFF loader, host side.
// Public surface of reference source/Mesh.h:16-142 (vertexPositions /
// vertexNormals / indexedTriangles / material / loadOFF / recomputeNormals), plus an extension the reference has no
// equivalent for: vertexColors and vertexUVs, filled by loadOFF from the colour and texture-coordinate variants of the
// format (COFF, STOFF, STCOFF), and sourceFile, the path loadOFF read.
// Acceleration data is not kept per mesh: the GPU context builds ONE flattened
// BVH over the whole scene (csrc/bvh_build.cpp), so computeAABB()/computeBVH()
// are accepted and do nothing.
#pragma once

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Material.h"
#include "Vec3.h"

typedef Vec3i Triangle;

class Mesh {
 public:
  Mesh() {}

  const std::vector<Vec3f>& vertexPositions() const { return m_vertexPositions; }
  std::vector<Vec3f>& vertexPositions() { return m_vertexPositions; }
  const std::vector<Vec3f>& vertexNormals() const { return m_vertexNormals; }
  std::vector<Vec3f>& vertexNormals() { return m_vertexNormals; }
  const std::vector<Triangle>& indexedTriangles() const { return m_indexedTriangles; }
  std::vector<Triangle>& indexedTriangles() { return m_indexedTriangles; }
  const Material& material() const { return m_material; }
  Material& material() { return m_material; }
  // one colour per vertex, or empty: the mesh has none (extension; RayTracer -vcolors renders with them)
  const std::vector<Vec3f>& vertexColors() const { return m_vertexColors; }
  std::vector<Vec3f>& vertexColors() { return m_vertexColors; }
  // one texture coordinate pair (s, t) per vertex, flattened [n][2], or empty: the mesh has none (extension; RayTracer
  // -textures renders with them)
  const std::vector<float>& vertexUVs() const { return m_vertexUVs; }
  std::vector<float>& vertexUVs() { return m_vertexUVs; }
  // the file loadOFF read last ("" before any): -textures looks for <stem>.ppm beside it
  const std::string& sourceFile() const { return m_sourceFile; }

  // Per-vertex normal = normalised sum of the unit normals of the incident
  // triangles (no area weighting), as reference Mesh.h:45-55.
  void recomputeNormals() {
    m_vertexNormals.resize(m_vertexPositions.size(), Vec3f());
    for (const Triangle& t : m_indexedTriangles) {
      const Vec3f& a = m_vertexPositions[t[0]];
      const Vec3f fn = normalize(cross(m_vertexPositions[t[1]] - a, m_vertexPositions[t[2]] - a));
      for (int c = 0; c < 3; ++c) m_vertexNormals[t[c]] += fn;
    }
    for (Vec3f& n : m_vertexNormals) n.normalize();
  }

  // Geomview OFF: header token, counts, vertices, then faces; polygons are fan
  // triangulated around their first vertex (reference Mesh.h:57-90).  The COFF header (extension): every vertex line
  // carries three or four colour values after its coordinates — integers 0..255 or, if any value of the file is written
  // with a point or an exponent, floats 0..1 — of which the fourth, the alpha, is ignored.  A value that is not a finite
  // decimal number >= 0, or an integer above 255, is refused (a float above 1 is kept: rt_material.albedo has no cap either).
  // The ST prefix (extension; Geomview's order of prefixes: STOFF, STCOFF): every vertex line ends in two texture
  // coordinates s t, behind the colour values where there are any; a coordinate that is not a finite decimal number is
  // refused, and so is a line with more or fewer values.
  void loadOFF(const std::string& filename) {
    m_vertexPositions.clear();
    m_indexedTriangles.clear();
    m_vertexColors.clear();
    m_vertexUVs.clear();
    m_sourceFile = filename;
    std::ifstream in(filename.c_str());
    if (!in) throw std::runtime_error("Error loading OFF file: " + filename);
    std::string magic;
    unsigned nv = 0, nf = 0, ne = 0;
    in >> magic;
    skipComment(in);
    in >> nv >> nf >> ne;
    skipComment(in);
    m_vertexPositions.resize(nv);
    const bool st = magic == "STOFF" || magic == "STCOFF", colours = magic == "COFF" || magic == "STCOFF";
    if (st || colours) readVertexAttributes(in, nv, colours, st, filename);
    else
    for (unsigned i = 0; i < nv; ++i) in >> m_vertexPositions[i];
    for (unsigned f = 0; f < nf; ++f) {
      unsigned corners = 0;
      in >> corners;
      std::vector<unsigned> idx(corners);
      for (unsigned c = 0; c < corners; ++c) in >> idx[c];
      for (unsigned c = 2; c < corners; ++c) m_indexedTriangles.push_back(Triangle(idx[0], idx[c - 1], idx[c]));
    }
    if (in.fail() && !in.eof()) throw std::runtime_error("Error Loading OFF file: malformed " + filename);
    recomputeNormals();
  }

  void computeAABB() {}
  void computeBVH() {}

 private:
  // plain decimal numbers only: strtod also reads nan, inf and hexadecimal floats
  static bool decimal(const std::string& tok, double* v) {
    char* end = nullptr;
    *v = std::strtod(tok.c_str(), &end);
    return end != tok.c_str() && *end == '\0' && tok.find_first_not_of("+-.0123456789eE") == std::string::npos && std::isfinite(*v);
  }

  // the nv vertex lines of a COFF, STOFF or STCOFF file: x y z [r g b [a]] [s t]
  void readVertexAttributes(std::ifstream& in, unsigned nv, bool colours, bool st, const std::string& filename) {
    std::vector<double> raw;
    bool floats = false;
    if (st) m_vertexUVs.resize(2 * static_cast<size_t>(nv));
    for (unsigned i = 0; i < nv; ++i) {
      in >> m_vertexPositions[i];
      std::string rest, tok;
      std::getline(in, rest);
      std::istringstream line(rest.substr(0, rest.find('#')));
      std::vector<std::string> toks;
      while (line >> tok) toks.push_back(tok);
      const size_t nCol = toks.size() - (st && toks.size() >= 2 ? 2 : 0);
      if (st && toks.size() < 2) throw std::runtime_error("Error Loading OFF file: an ST vertex needs two texture coordinates in " + filename);
      if (colours ? nCol != 3 && nCol != 4 : nCol != 0)
        throw std::runtime_error(std::string("Error Loading OFF file: ") +
                                 (colours ? "a COFF vertex needs 3 or 4 colour values" : "an STOFF vertex needs exactly two texture coordinates") +
                                 " in " + filename);
      for (size_t n = 0; n < nCol; ++n) {
        double v;
        if (!decimal(toks[n], &v) || v < 0.)
          throw std::runtime_error("Error Loading OFF file: colour value '" + toks[n] + "' is not a finite number >= 0 in " + filename);
        floats = floats || toks[n].find_first_of(".eE") != std::string::npos;
        if (n < 3) raw.push_back(v);
      }
      for (size_t n = 0; st && n < 2; ++n) {
        double v;
        if (!decimal(toks[nCol + n], &v))
          throw std::runtime_error("Error Loading OFF file: texture coordinate '" + toks[nCol + n] + "' is not a finite number in " + filename);
        m_vertexUVs[2 * static_cast<size_t>(i) + n] = static_cast<float>(v);
      }
    }
    if (!colours) return;
    if (!floats)
      for (double v : raw)
        if (v > 255.) throw std::runtime_error("Error Loading OFF file: an integer colour value above 255 in " + filename);
    m_vertexColors.resize(nv);
    for (unsigned i = 0; i < nv; ++i)
      for (int c = 0; c < 3; ++c)
        m_vertexColors[i][c] = floats ? static_cast<float>(raw[3 * i + c]) : static_cast<float>(raw[3 * i + c]) / 255.f;
  }

  static void skipComment(std::ifstream& in) {
    while (in.peek() == '\n' || in.peek() == ' ' || in.peek() == '\r') in.get();
    if (in.peek() == '#') {
      std::string rest;
      std::getline(in, rest);
    }
  }

  std::vector<Vec3f> m_vertexPositions;
  std::vector<Vec3f> m_vertexNormals;
  std::vector<Triangle> m_indexedTriangles;
  std::vector<Vec3f> m_vertexColors;
  std::vector<float> m_vertexUVs;
  std::string m_sourceFile;
  Material m_material;
};
