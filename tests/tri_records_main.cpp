// tri_records_main.cpp -- the host side of the set-up records (rusterix_amd/csrc/rxr_host_setup.h: the fetch out of a frame blob's sections
// and rxr_tri_records, the one definition of a TriSetup / TriShade pair) as a program of its own: tests/test_tri_records_cpu.py feeds it
// small frames full of special values and compares what it writes with numpy float32 restatements of the reference's expressions.
// Built with a host compiler (-O2 -ffp-contract=off), and once more with -fsanitize=address,undefined: every section is its own heap
// block of exactly its size, so an index that strays is caught.
//
//   tri_records_main IN OUT
// IN:  nine words -- n_verts, n_tris, n_batches, n_tex, edgeless, has_clip, sample_mode, width, height -- then the sections in the order
//      of HostSetupSource: pv, uv, nrm, idx, edges (a record, or with `edgeless` a word, per triangle), tri_info, batches, tex, clip.
// OUT: per triangle one word "can produce a pixel", the 24 words of its TriSetup and the 20 of its TriShade.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../rusterix_amd/csrc/rxr_host_setup.h"

template <class T> static std::unique_ptr<T[]> section(FILE *f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);  // (n == 0: a block of no bytes -- nothing may be read from it)
    if (n && fread(p.get(), sizeof(T), n, f) != n) {
        fprintf(stderr, "tri_records_main: input too short\n");
        exit(2);
    }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::unique_ptr<uint32_t[]> head = section<uint32_t>(f, 9);
    const size_t nv = head[0], nt = head[1], nb = head[2], ntex = head[3];
    const bool edgeless = head[4] != 0, has_clip = head[5] != 0;
    const auto pv = section<float>(f, 4 * nv), uv = section<float>(f, 2 * nv), nrm = section<float>(f, 3 * nv);
    const auto idx = section<uint32_t>(f, 3 * nt);
    const auto edge_words = section<uint32_t>(f, edgeless ? nt : 0);
    const auto edge_records = section<rxr_edges>(f, edgeless ? 0 : nt);
    const auto tri_info = section<uint32_t>(f, 2 * nt);
    const auto batches = section<DevBatch>(f, nb);
    const auto tex = section<DevTexDesc>(f, ntex);
    const auto clip = section<uint32_t>(f, has_clip ? 4 * nb : 0);
    fclose(f);

    HostSetupSource src{};
    src.pv = pv.get();
    src.uv = uv.get();
    src.nrm = nrm.get();
    src.idx = idx.get();
    src.edges = edgeless ? (const void *)edge_words.get() : (const void *)edge_records.get();
    src.edgeless = edgeless;
    src.tri_info = tri_info.get();
    src.batches = batches.get();
    src.tex = tex.get();
    src.clip = has_clip ? clip.get() : nullptr;
    src.sample_mode = head[6];
    src.width = head[7];
    src.height = head[8];

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (size_t t = 0; t < nt; ++t) {
        TriSetup S{};
        TriShade H{};
        const uint32_t live = rxr_host_tri_records(src, t, S, H) ? 1u : 0u;
        fwrite(&live, 4, 1, o);
        fwrite(&S, sizeof(S), 1, o);
        fwrite(&H, sizeof(H), 1, o);
    }
    fclose(o);
    return 0;
}
