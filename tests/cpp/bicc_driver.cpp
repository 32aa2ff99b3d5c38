// graphlily::app::BiconnectedComponents driven from C++: the block labels, the blocks per vertex and the 2-edge-connected
// components are written as raw 32-bit words for tests/test_gpu_bicc.py to compare with the Python driver's, the counts are
// printed, and what ties the outputs together is checked here: a label is an entry of its own block and at most the entry it
// labels, the distinct labels are num_blocks(), the labels with two entries num_bridges(), the vertices with two or more blocks
// num_articulation_points(), and vertex_blocks()[v] is the number of distinct labels in row v.
//   bicc_driver graph.npz out_dir
//   g++ -std=c++11 -I<repo>/include tests/cpp/bicc_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/bicc.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

static bool write_words(const std::string &path, const uint32_t *data, size_t count) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(data, sizeof(uint32_t), count, f) != count) { printf("cannot write %s\n", path.c_str()); return false; }
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::BiconnectedComponents bc(graphlily::num_hbm_channels, 1024, 256);
    bc.set_target("hw");
    bc.set_up_runtime("unused.xclbin");
    bc.load_and_format_matrix(npz, true);
    bc.send_matrix_host_to_device();
    auto block = bc.run(true);
    int bad = 0;
    const size_t nnz = bc.graph().adj_indices.size(), n = bc.num_vertices();
    if (block.size() != nnz || bc.vertex_blocks().size() != n || bc.edge_components().size() != n) { printf("size mismatch\n"); return 1; }
    std::vector<uint32_t> entries(nnz, 0);
    unsigned long long checksum = 0, articulation = 0;
    for (size_t v = 0; v < n; v++) {
        std::set<uint32_t> mine;
        for (uint32_t j = bc.graph().adj_indptr[v]; j < bc.graph().adj_indptr[v + 1]; j++) {
            if ((block[j] > j || block[block[j]] != block[j]) && bad++ < 5) printf("entry %u is given block %u\n", j, block[j]);
            if (block[j] < nnz) entries[block[j]]++;
            mine.insert(block[j]);
            checksum = checksum * 1000003ull + block[j] + 1ull;    // (mod 2^64: tests/test_gpu_bicc.py computes the same)
        }
        if (mine.size() != bc.vertex_blocks()[v] && bad++ < 5)
            printf("vertex %zu lies in %zu blocks, vertex_blocks() says %u\n", v, mine.size(), bc.vertex_blocks()[v]);
        articulation += bc.vertex_blocks()[v] >= 2 ? 1 : 0;
        if (bc.edge_components()[v] > v && bad++ < 5) printf("vertex %zu has edge component %u, which is above it\n", v, bc.edge_components()[v]);
    }
    unsigned long long blocks = 0, bridges = 0;
    for (size_t j = 0; j < nnz; j++) {
        blocks += entries[j] ? 1 : 0;
        bridges += entries[j] == 2 ? 1 : 0;
    }
    if (blocks != bc.num_blocks()) { printf("%llu distinct labels, num_blocks() = %llu\n", blocks, (unsigned long long)bc.num_blocks()); bad++; }
    if (bridges != bc.num_bridges()) { printf("%llu blocks of one edge, num_bridges() = %llu\n", bridges, (unsigned long long)bc.num_bridges()); bad++; }
    if (articulation != bc.num_articulation_points()) {
        printf("%llu vertices in two blocks or more, num_articulation_points() = %llu\n", articulation, (unsigned long long)bc.num_articulation_points());
        bad++;
    }
    if (!write_words(out + "/cpp_block.bin", block.data(), nnz) || !write_words(out + "/cpp_vertex_blocks.bin", bc.vertex_blocks().data(), n) ||
        !write_words(out + "/cpp_edge_component.bin", bc.edge_components().data(), n))
        return 2;
    printf("blocks: %llu\narticulation points: %llu\nbridges: %llu\ntrees: %llu\ndepth: %llu\nchecksum: %llu\n", (unsigned long long)bc.num_blocks(),
           (unsigned long long)bc.num_articulation_points(), (unsigned long long)bc.num_bridges(), (unsigned long long)bc.num_trees(),
           (unsigned long long)bc.depth(), checksum);
    if (!bad) printf("BiconnectedComponents::run OK\n");
    return bad ? 1 : 0;
}
