// Mesh.h — indexed triangle mesh container + OFF loader, host side.
// Public surface of reference source/Mesh.h:16-142 (vertexPositions /
// vertexNormals / indexedTriangles / material / loadOFF / recomputeNormals), plus an extension the reference has no
// equivalent for: vertexColors, filled by loadOFF from the colour variant of the format (COFF).
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
  void loadOFF(const std::string& filename) {
    m_vertexPositions.clear();
    m_indexedTriangles.clear();
    m_vertexColors.clear();
    std::ifstream in(filename.c_str());
    if (!in) throw std::runtime_error("Error loading OFF file: " + filename);
    std::string magic;
    unsigned nv = 0, nf = 0, ne = 0;
    in >> magic;
    skipComment(in);
    in >> nv >> nf >> ne;
    skipComment(in);
    m_vertexPositions.resize(nv);
    if (magic == "COFF") readColoredVertices(in, nv, filename);
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
  // the nv vertex lines of a COFF file: x y z r g b [a]
  void readColoredVertices(std::ifstream& in, unsigned nv, const std::string& filename) {
    std::vector<double> raw;
    bool floats = false;
    for (unsigned i = 0; i < nv; ++i) {
      in >> m_vertexPositions[i];
      std::string rest, tok;
      std::getline(in, rest);
      std::istringstream line(rest.substr(0, rest.find('#')));
      unsigned n = 0;
      while (line >> tok) {
        char* end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        // plain decimal numbers only: strtod also reads nan, inf and hexadecimal floats
        if (end == tok.c_str() || *end != '\0' || tok.find_first_not_of("+-.0123456789eE") != std::string::npos || !std::isfinite(v) || v < 0.)
          throw std::runtime_error("Error Loading OFF file: colour value '" + tok + "' is not a finite number >= 0 in " + filename);
        floats = floats || tok.find_first_of(".eE") != std::string::npos;
        if (n < 3) raw.push_back(v);
        ++n;
      }
      if (n != 3 && n != 4) throw std::runtime_error("Error Loading OFF file: a COFF vertex needs 3 or 4 colour values in " + filename);
    }
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
  Material m_material;
};
