// cpp_cell_proofs_at_runner -- drives Kzg::compute_cell_kzg_proofs_at and Kzg::compute_cell_kzg_proofs_at_many of the C++ mirror
// (include/kzg355.hpp) for tests/test_gpu_cell_proofs_at.py.
//   usage: cpp_cell_proofs_at_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <blobs.bin> <counts.bin> <indices.bin> <out.bin> [single]
//   blobs.bin: the blobs (131072 bytes each) back to back; counts.bin: the number of indices per blob, one byte each; indices.bin: the blobs'
//   cell indices back to back, one byte each.  "single": one compute_cell_kzg_proofs_at call per blob instead of one _many call.
//   out.bin: per computed blob its chosen cells (2048 bytes each) then their proofs (48 bytes each); prints one line per blob: "ok" | "err <kind>"
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include "../../include/kzg355.hpp"

using namespace kzg355;

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc < 7) { std::cerr << "usage: cpp_cell_proofs_at_runner <g1.bin> <g2.bin> <blobs.bin> <counts.bin> <indices.bin> <out.bin> [single]\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), in = slurp(argv[3]), counts = slurp(argv[4]), ix = slurp(argv[5]);
    const bool single = argc > 7 && !std::strcmp(argv[7], "single");
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    if (counts.size() * BYTES_PER_BLOB != in.size()) { std::cerr << "counts.bin and blobs.bin disagree\n"; return 2; }
    std::vector<Blob> blobs;
    std::vector<std::vector<size_t>> lists;
    size_t at = 0;
    for (size_t b = 0; b < counts.size(); b++) {
        if (at + counts[b] > ix.size()) { std::cerr << "counts.bin asks for more than indices.bin holds\n"; return 2; }
        blobs.push_back(Blob::from_bytes(&in[b * BYTES_PER_BLOB], BYTES_PER_BLOB).value());
        lists.emplace_back(ix.begin() + at, ix.begin() + at + counts[b]);
        at += counts[b];
    }
    std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>> res;
    if (single) for (size_t b = 0; b < blobs.size(); b++) res.push_back(Kzg::compute_cell_kzg_proofs_at(blobs[b], lists[b], s));
    else {
        auto r = Kzg::compute_cell_kzg_proofs_at_many(blobs, lists, s);
        if (r.is_err()) { std::cerr << "call error " << r.error().kind << "\n"; return 1; }
        res = r.value();
    }
    std::ofstream out(argv[6], std::ios::binary);
    for (const auto &u : res) {
        if (u.is_err()) { std::cout << "err " << u.error().kind << "\n"; continue; }
        for (const Cell &c : u.value().first) out.write(reinterpret_cast<const char *>(c.data()), KZG355_BYTES_PER_CELL);
        for (const KzgProof &p : u.value().second) out.write(reinterpret_cast<const char *>(p.data()), 48);
        std::cout << "ok\n";
    }
    return 0;
}
