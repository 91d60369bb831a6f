// Native reader of ASCII OFF and Wavefront OBJ triangle meshes (host) for generate_dataset: the reference reads its ModelNet meshes
// with open3d's read_triangle_mesh (generate_dataset.py:9).  Count-then-fill like ply.cpp: a first call with NULL buffers returns the
// sizes, a second fills the caller's arrays.  Polygons are fan-triangulated (v0, vi, vi+1).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/pcgc_hip.h"

namespace {

enum { MESH_OK = 0, MESH_NO_FILE = -1, MESH_MALFORMED = -3, MESH_BAD_INDEX = -4, MESH_TOO_SMALL = -5 };

struct Mesh { std::vector<double> v; std::vector<int64_t> f; };

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\f' || c == '\v'; }

// whitespace-separated tokens of a buffer; '#' starts a comment that runs to the end of its line
struct Tokens {
    const char* p; const char* end;
    void skip_blank() {                                  // blanks, newlines and comments
        while (p < end) {
            if (*p == '#') { while (p < end && *p != '\n') ++p; }
            else if (is_space(*p) || *p == '\n') ++p;
            else break;
        }
    }
    void skip_line() { while (p < end && *p != '\n') ++p; }
    bool next(const char*& b, const char*& e) {
        skip_blank();
        if (p >= end) return false;
        b = p;
        while (p < end && !is_space(*p) && *p != '\n' && *p != '#') ++p;
        e = p;
        return true;
    }
};

bool to_double(const char* b, const char* e, double& out) {
    if (b >= e || e - b > 63) return false;
    char tmp[64]; std::memcpy(tmp, b, (size_t)(e - b)); tmp[e - b] = '\0';
    char* stop = nullptr;
    out = std::strtod(tmp, &stop);
    return stop != tmp && *stop == '\0';
}

bool to_int(const char* b, const char* e, int64_t& out) {
    if (b >= e || e - b > 20) return false;
    char tmp[24]; std::memcpy(tmp, b, (size_t)(e - b)); tmp[e - b] = '\0';
    char* stop = nullptr; errno = 0;
    const long long v = std::strtoll(tmp, &stop, 10);
    if (stop == tmp || *stop != '\0' || errno == ERANGE) return false;
    out = v; return true;
}

void fan(Mesh& m, const std::vector<int64_t>& poly) {
    for (size_t i = 1; i + 1 < poly.size(); ++i) { m.f.push_back(poly[0]); m.f.push_back(poly[i]); m.f.push_back(poly[i + 1]); }
}

// OFF: "OFF" then nv nf ne — on the next line, on the same line, or glued to the keyword ("OFF8 6 0", as many ModelNet40 files have it);
// nv lines "x y z ..." and nf lines "k i0 .. ik-1 ..." (anything after the needed numbers of a line, e.g. colours, is ignored)
int parse_off(const char* buf, size_t size, Mesh& m) {
    Tokens t{buf, buf + size};
    const char *b, *e;
    if (!t.next(b, e) || e - b < 3 || std::strncmp(b, "OFF", 3) != 0) return MESH_MALFORMED;
    int64_t head[3]; int have = 0;
    if (e - b > 3) { if (!to_int(b + 3, e, head[have++])) return MESH_MALFORMED; }
    while (have < 3) { if (!t.next(b, e) || !to_int(b, e, head[have++])) return MESH_MALFORMED; }
    const int64_t nv = head[0], nf = head[1];
    if (nv < 0 || nf < 0 || nv > 0x7FFFFFFFll || nf > 0x7FFFFFFFll) return MESH_MALFORMED;
    t.skip_line();
    m.v.reserve((size_t)nv * 3);
    for (int64_t i = 0; i < nv; ++i) {
        for (int c = 0; c < 3; ++c) {
            double x;
            if (!t.next(b, e) || !to_double(b, e, x)) return MESH_MALFORMED;
            m.v.push_back(x);
        }
        t.skip_line();
    }
    std::vector<int64_t> poly;
    for (int64_t i = 0; i < nf; ++i) {
        int64_t k;
        if (!t.next(b, e) || !to_int(b, e, k) || k < 0 || k > (1 << 20)) return MESH_MALFORMED;
        poly.clear();
        for (int64_t j = 0; j < k; ++j) {
            int64_t idx;
            if (!t.next(b, e) || !to_int(b, e, idx)) return MESH_MALFORMED;
            if (idx < 0 || idx >= nv) return MESH_BAD_INDEX;
            poly.push_back(idx);
        }
        t.skip_line();
        fan(m, poly);
    }
    return MESH_OK;
}

// OBJ: "v x y z [w]" and "f t t t ..." with t = a, a/b, a/b/c or a//c; a is 1-based, or negative = counted back from the vertices read so
// far.  Every other record (vn, vt, g, o, s, usemtl, mtllib, comments ...) is skipped.
int parse_obj(const char* buf, size_t size, Mesh& m) {
    const char* p = buf; const char* end = buf + size;
    std::vector<int64_t> poly;
    std::vector<int64_t> positive;                       // forward references are checked once every vertex is known
    while (p < end) {
        const char* eol = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        const char* le = eol ? eol : end;
        Tokens t{p, le};
        const char *b, *e;
        if (t.next(b, e)) {
            if (e - b == 1 && *b == 'v') {
                for (int c = 0; c < 3; ++c) {
                    double x;
                    if (!t.next(b, e) || !to_double(b, e, x)) return MESH_MALFORMED;
                    m.v.push_back(x);
                }
            } else if (e - b == 1 && *b == 'f') {
                const int64_t nv = (int64_t)(m.v.size() / 3);
                poly.clear();
                while (t.next(b, e)) {
                    const char* slash = (const char*)std::memchr(b, '/', (size_t)(e - b));
                    int64_t a;
                    if (!to_int(b, slash ? slash : e, a)) return MESH_MALFORMED;
                    if (a == 0) return MESH_BAD_INDEX;
                    if (a < 0) { a += nv; if (a < 0) return MESH_BAD_INDEX; }
                    else { a -= 1; positive.push_back(a); }
                    poly.push_back(a);
                }
                if (poly.size() < 3) return MESH_MALFORMED;
                fan(m, poly);
            }
        }
        p = eol ? eol + 1 : end;
    }
    const int64_t nv = (int64_t)(m.v.size() / 3);
    for (int64_t a : positive) if (a >= nv) return MESH_BAD_INDEX;
    return MESH_OK;
}

bool ends_with_nocase(const char* s, const char* ext) {
    const size_t n = std::strlen(s), k = std::strlen(ext);
    if (n < k) return false;
    for (size_t i = 0; i < k; ++i) { char c = s[n - k + i]; if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a'); if (c != ext[i]) return false; }
    return true;
}

}  // namespace

// counts[0] = vertices, counts[1] = triangles.  verts / faces NULL: sizes only.  0 ok; -1 the file cannot be read; -3 malformed (or
// truncated, or neither .off / .obj nor an OFF keyword at its start); -4 a face names a vertex that does not exist; -5 buffers too small.
extern "C" int pcgc_mesh_read(const char* path, double* verts, int64_t vcap, int32_t* faces, int64_t fcap, int64_t* counts) {
    if (!path || !counts) return MESH_MALFORMED;
    counts[0] = counts[1] = 0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return MESH_NO_FILE;
    std::fseek(f, 0, SEEK_END); const long size = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    if (size < 0) { std::fclose(f); return MESH_NO_FILE; }
    std::vector<char> buf((size_t)size + 1);
    if (size > 0 && std::fread(buf.data(), 1, (size_t)size, f) != (size_t)size) { std::fclose(f); return MESH_NO_FILE; }
    std::fclose(f);
    Mesh m;
    int rc;
    if (ends_with_nocase(path, ".obj")) rc = parse_obj(buf.data(), (size_t)size, m);
    else rc = parse_off(buf.data(), (size_t)size, m);          // (.off, and anything else must open with the OFF keyword)
    if (rc != MESH_OK) return rc;
    const int64_t nv = (int64_t)(m.v.size() / 3), nt = (int64_t)(m.f.size() / 3);
    if (nv > 0x7FFFFFFFll || nt > 0x7FFFFFFFll) return MESH_MALFORMED;
    counts[0] = nv; counts[1] = nt;
    if (!verts && !faces) return MESH_OK;
    if (!verts || !faces || vcap < nv || fcap < nt) return MESH_TOO_SMALL;
    if (nv) std::memcpy(verts, m.v.data(), (size_t)nv * 3 * sizeof(double));
    for (int64_t i = 0; i < 3 * nt; ++i) faces[i] = (int32_t)m.f[(size_t)i];
    return MESH_OK;
}
