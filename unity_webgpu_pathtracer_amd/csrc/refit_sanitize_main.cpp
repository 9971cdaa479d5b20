// refit_sanitize_main.cpp — the host CWBVH build and refit as a stand-alone program for sanitizer runs (make refit-sanitize:
// -fsanitize=address,undefined over bvh_builder.cpp and bvh_refit.cpp; tests/test_refit.py runs it).
// usage: refit_sanitize build-vertices.bin refit-vertices.bin expected-nodes.bin expected-tris.bin (raw float4 / byte arrays)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "bvh_builder.h"
#include "bvh_refit.h"

static std::vector<char> slurp(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s build.bin refit.bin nodes.bin tris.bin\n", argv[0]); return 2; }
    const std::vector<char> v = slurp(argv[1]), w = slurp(argv[2]), nodes = slurp(argv[3]), tris = slurp(argv[4]);
    if (v.empty() || v.size() % 48 || w.size() != v.size()) { fprintf(stderr, "bad vertex files\n"); return 2; }
    const uint32_t n = (uint32_t)(v.size() / 48);
    std::vector<PTFloat4> vb(n * 3), wb(n * 3);                  // exact-size heap copies: an overread is a report
    memcpy(vb.data(), v.data(), v.size());
    memcpy(wb.data(), w.data(), w.size());
    ptbvh::Cwbvh bvh;
    if (!bvh.build(vb.data(), n)) { fprintf(stderr, "build failed\n"); return 1; }
    std::vector<PTFloat4> bn(bvh.nodeData.begin(), bvh.nodeData.begin() + bvh.usedBlocks), bt(bvh.triData.begin(), bvh.triData.begin() + (size_t)n * 3);
    std::string err;
    if (!ptbvh::refit_cwbvh(bn.data(), bn.size() / 5, bt.data(), bt.size(), 0, 0, wb.data(), n, err)) { fprintf(stderr, "refit failed: %s\n", err.c_str()); return 1; }
    if (bn.size() * 16 != nodes.size() || memcmp(bn.data(), nodes.data(), nodes.size())) { fprintf(stderr, "node bytes differ\n"); return 1; }
    if (bt.size() * 16 != tris.size() || memcmp(bt.data(), tris.data(), tris.size())) { fprintf(stderr, "triangle bytes differ\n"); return 1; }
    // a refused input must be refused cleanly too: a child index far outside the array
    uint32_t far = 0xFFFFFF00u, meta = (1u << 5) | 24u;
    memcpy(&bn[1].x, &far, 4);
    memcpy(&bn[1].z, &meta, 4);
    if (ptbvh::refit_cwbvh(bn.data(), bn.size() / 5, bt.data(), bt.size(), 0, 0, wb.data(), n, err)) { fprintf(stderr, "a broken tree was accepted\n"); return 1; }
    printf("refit ok: %u triangles, %zu nodes\n", n, bn.size() / 5);
    return 0;
}
