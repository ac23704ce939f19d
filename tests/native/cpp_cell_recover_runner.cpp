// cpp_cell_recover_runner -- drives Kzg::recover_cells_and_kzg_proofs of the C++ mirror (include/kzg355.hpp) for tests/test_gpu_cell_recover.py.
//   usage: cpp_cell_recover_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <indices.bin> <cells.bin> <out.bin>
//   indices.bin: n cell indices, one byte each; cells.bin: rows of n cells (2048 bytes each) back to back, one row per blob
//   out.bin: per row the 128 cells (2048 bytes each) then the 128 proofs (48 bytes each); prints one line per row: "ok" | "err <kind>"
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
    if (argc < 6) { std::cerr << "usage: cpp_cell_recover_runner <g1.bin> <g2.bin> <indices.bin> <cells.bin> <out.bin>\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), ix = slurp(argv[3]), in = slurp(argv[4]);
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    const std::vector<size_t> indices(ix.begin(), ix.end());
    const size_t n = indices.size(), row = n * KZG355_BYTES_PER_CELL;
    if (n == 0) { std::cerr << "no indices\n"; return 2; }
    std::ofstream out(argv[5], std::ios::binary);
    for (size_t at = 0; at + row <= in.size(); at += row) {
        std::vector<Cell> cells;
        for (size_t i = 0; i < n; i++) cells.push_back(Cell::from_bytes(&in[at + i * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
        auto r = Kzg::recover_cells_and_kzg_proofs(indices, cells, s);
        if (r.is_err()) { std::cout << "err " << r.error().kind << "\n"; continue; }
        for (const Cell &c : r.value().first) out.write(reinterpret_cast<const char *>(c.data()), KZG355_BYTES_PER_CELL);
        for (const KzgProof &p : r.value().second) out.write(reinterpret_cast<const char *>(p.data()), 48);
        std::cout << "ok\n";
    }
    return 0;
}
