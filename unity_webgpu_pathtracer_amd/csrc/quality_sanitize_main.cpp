// quality_sanitize_main.cpp — the host tree-quality measure as a stand-alone program for sanitizer runs (make quality-sanitize:
// -fsanitize=address,undefined over bvh_quality.cpp and bvh_refit.cpp; tests/test_geometry_quality.py runs it).
// usage: quality_sanitize nodes.bin tris.bin (raw byte arrays); prints the numbers, one line
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "bvh_quality.h"

static std::vector<char> slurp(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s nodes.bin tris.bin\n", argv[0]); return 2; }
    const std::vector<char> nodes = slurp(argv[1]), tris = slurp(argv[2]);
    if (nodes.empty() || nodes.size() % 80 || tris.empty() || tris.size() % 48) { fprintf(stderr, "bad array files\n"); return 2; }
    std::vector<PTFloat4> bn(nodes.size() / 16), bt(tris.size() / 16);      // exact-size heap copies: an overread is a report
    memcpy(bn.data(), nodes.data(), nodes.size());
    memcpy(bt.data(), tris.data(), tris.size());
    const uint32_t n = (uint32_t)(tris.size() / 48);
    ptbvh::Quality q;
    std::string err;
    if (!ptbvh::measure_cwbvh(bn.data(), bn.size() / 5, bt.data(), bt.size(), n, q, err)) { fprintf(stderr, "measure failed: %s\n", err.c_str()); return 1; }
    // what is refused must be refused cleanly too: the wrong triangle count, then a child index far outside the array
    ptbvh::Quality r;
    if (n > 1 && ptbvh::measure_cwbvh(bn.data(), bn.size() / 5, bt.data(), bt.size() - 3, n - 1, r, err)) { fprintf(stderr, "a wrong triangle count was accepted\n"); return 1; }
    uint32_t far = 0xFFFFFF00u, meta = (1u << 5) | 24u;
    memcpy(&bn[1].x, &far, 4);
    memcpy(&bn[1].z, &meta, 4);
    if (ptbvh::measure_cwbvh(bn.data(), bn.size() / 5, bt.data(), bt.size(), n, r, err)) { fprintf(stderr, "a broken tree was accepted\n"); return 1; }
    printf("quality ok: %u triangles, %u nodes, %u levels, root half area %.17g, cost %.17g\n", q.triangleCount, q.nodeCount, q.levels, q.rootHalfArea, q.sahCost);
    return 0;
}
