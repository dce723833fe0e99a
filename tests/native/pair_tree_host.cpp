// Host driver of csrc/host/pair_tree.cpp for tests/test_pair_tree_host.py: the host half of a scene
// upload, run without a device.
//
//   pair_tree_host <layout request, -1..3> <in.bin> <out prefix>
//
// in.bin: int32 {ntri, nnodes, nmat, has_tri_id}, then float32 v0, v1, v2, n0, n1, n2 (3 ntri each),
// int32 mat (ntri), int32 tri_id (ntri, if has_tri_id), float32 bmin, bmax (3 nnodes each), int32 offset,
// nprims (nnodes each).  Writes <prefix>.pairs / .quads (float32), .src (uint32), .tri / .sh (float32) and
// prints one info line; a rejected desc prints "error: <message>" and writes nothing.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/pair_tree.hpp"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool write_all(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int request = atoi(argv[1]);
    const std::string prefix = argv[3];
    FILE* f = fopen(argv[2], "rb");
    int32_t h[4];
    if (!f || fread(h, 4, 4, f) != 4 || h[0] < 0 || h[1] < 0) return 2;
    const size_t T = (size_t)h[0], N = (size_t)h[1];
    std::vector<float> v[6], bmin, bmax;
    std::vector<int32_t> mat, tri_id, offset, nprims;
    bool ok = true;
    for (auto& a : v) ok = ok && read_n(f, a, 3 * T);
    ok = ok && read_n(f, mat, T) && read_n(f, tri_id, h[3] ? T : 0) && read_n(f, bmin, 3 * N) && read_n(f, bmax, 3 * N) &&
         read_n(f, offset, N) && read_n(f, nprims, N);
    fclose(f);
    if (!ok) return 2;
    mcpt_scene_desc d{};
    d.ntri = h[0];
    d.v0 = v[0].data(), d.v1 = v[1].data(), d.v2 = v[2].data(), d.n0 = v[3].data(), d.n1 = v[4].data(), d.n2 = v[5].data();
    d.mat = mat.data();
    d.tri_id = h[3] ? tri_id.data() : nullptr;
    d.nnodes = h[1];
    d.bmin = bmin.data(), d.bmax = bmax.data(), d.offset = offset.data(), d.nprims = nprims.data();
    d.nmat = h[2];

    mcpt_host::PairTree pt;
    std::string err;
    if (!mcpt_host::build_pair_tree(d, request, pt, err)) {
        printf("error: %s\n", err.c_str());
        return 0;
    }
    std::vector<float4> tri, sh, quads;
    std::vector<uint32_t> src;
    int quad_root = 0, max_push = 0;
    mcpt_host::pack_records(d, tri, sh);
    if (d.ntri > 0) mcpt_host::pairs_to_quads(pt.pairs, pt.root_ref, quads, quad_root, max_push, src);  // as an upload: never of an empty tree
    if (!write_all(prefix + ".pairs", pt.pairs) || !write_all(prefix + ".quads", quads) || !write_all(prefix + ".src", src) ||
        !write_all(prefix + ".tri", tri) || !write_all(prefix + ".sh", sh))
        return 2;
    printf("ok npairs=%zu root_ref=%d depth=%d layout=%d contained=%d nested=%d tri_f4=%d nquads=%zu quad_root=%d max_push=%d\n",
           pt.pairs.size() / 4, pt.root_ref, pt.depth, pt.layout, (int)pt.contained, (int)pt.nested, mcpt_dev::kTriF4,
           quads.size() / 8, quad_root, max_push);
    return 0;
}
