// oracle/asan_stack_overflow.cpp — stand-alone sanitizer run of the oracle's walks on the deep-stack cases (make -C oracle asan-stack-test).
//
// Linked with pt_oracle.cpp under -fsanitize=address,undefined: traces the rays of tests/golden/stack_overflow_cases.bin (written by
// tests/stack_cases.py: deep_cwbvh(40) and deep_tlas(48), both ray families each) through oracle_trace_rays and compares every record,
// bit for bit, and the batch's stackOverflows with the expectations stored beside them.  More than 32 pending entries are exactly
// where a traversal stack can be indexed out of bounds; the sanitizers report that, the comparison reports a wrong overflow rule.
//
// File: "PTSO", u32 case count; per case u32 features, u32 tlasIndexOffset, u64 expected stackOverflows, then eight blobs (u64 byte
// count + bytes): nodes, triangle rows, attribute records, materials, TLAS data, instances, rays (OracleRay), expected records (float4).
#include <cstdio>
#include <cstring>
#include <vector>

#include "pt_oracle.h"

namespace {
bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
} // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s stack_overflow_cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    uint32_t cases = 0;
    if (!read_exact(f, magic, 4) || memcmp(magic, "PTSO", 4) != 0 || !read_exact(f, &cases, 4)) { fprintf(stderr, "bad header\n"); return 2; }
    int failures = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t features = 0, tlasIndexOffset = 0;
        uint64_t overflows = 0;
        if (!read_exact(f, &features, 4) || !read_exact(f, &tlasIndexOffset, 4) || !read_exact(f, &overflows, 8)) { fprintf(stderr, "truncated\n"); return 2; }
        std::vector<unsigned char> blob[8];
        for (auto& b : blob) {
            uint64_t n = 0;
            if (!read_exact(f, &n, 8) || n > (64u << 20)) { fprintf(stderr, "truncated\n"); return 2; }
            b.resize((size_t)n);
            if (!read_exact(f, b.data(), b.size())) { fprintf(stderr, "truncated\n"); return 2; }
        }
        PTSceneDesc d;
        memset(&d, 0, sizeof(d));
        d.bvhNodes = blob[0].data(); d.bvhNodesBytes = blob[0].size();
        d.bvhTris = blob[1].data(); d.bvhTrisBytes = blob[1].size();
        d.triAttrs = blob[2].data(); d.triAttrsBytes = blob[2].size();
        d.materials = blob[3].data(); d.materialCount = (uint32_t)(blob[3].size() / 128);
        d.features = features;
        if (features & PT_FEATURE_HAS_TLAS) {
            d.tlasData = (const float*)blob[4].data(); d.tlasDataFloats = blob[4].size() / 4;
            d.tlasIndexOffset = tlasIndexOffset;
            d.gpuInstances = blob[5].data(); d.instanceCount = (uint32_t)(blob[5].size() / 144);
        }
        const uint64_t n = blob[6].size() / sizeof(OracleRay);
        if (blob[7].size() != n * 16) { fprintf(stderr, "case %u: %zu expected bytes for %llu rays\n", c, blob[7].size(), (unsigned long long)n); return 2; }
        std::vector<float> out(n * 4);
        PTStats st;
        if (oracle_trace_rays(&d, (const OracleRay*)blob[6].data(), n, out.data(), &st) != 0) { fprintf(stderr, "case %u: oracle_trace_rays failed\n", c); return 2; }
        uint64_t bad = 0, hits = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (memcmp(&out[i * 4], blob[7].data() + i * 16, 16) != 0) bad++;
            uint32_t prim;
            memcpy(&prim, &out[i * 4 + 3], 4);
            hits += prim != 0xFFFFFFFFu;
        }
        printf("case %u: %llu rays, %llu hits, %llu records differ, stackOverflows %llu (expected %llu)\n", c, (unsigned long long)n,
               (unsigned long long)hits, (unsigned long long)bad, (unsigned long long)st.stackOverflows, (unsigned long long)overflows);
        if (bad || st.stackOverflows != overflows) failures++;
    }
    fclose(f);
    return failures ? 1 : 0;
}
