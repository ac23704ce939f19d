// cpp_cell_recover_sets_runner -- drives Kzg::recover_cells_and_kzg_proofs_many_sets of the C++ mirror (include/kzg355.hpp) for
// tests/test_gpu_cell_recover_sets.py.
//   usage: cpp_cell_recover_sets_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <counts.bin> <indices.bin> <cells.bin> <out.bin>
//   counts.bin: the number of known cells per unit, one byte each; indices.bin: the units' cell indices back to back, one byte each;
//   cells.bin: the units' cells (2048 bytes each) back to back, in the order of the indices
//   out.bin: per recovered unit the 128 cells (2048 bytes each) then the 128 proofs (48 bytes each); prints one line per unit: "ok" | "err <kind>"
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
    if (argc < 7) { std::cerr << "usage: cpp_cell_recover_sets_runner <g1.bin> <g2.bin> <counts.bin> <indices.bin> <cells.bin> <out.bin>\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), counts = slurp(argv[3]), ix = slurp(argv[4]), in = slurp(argv[5]);
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    std::vector<Kzg::RecoverUnit> units;
    size_t at = 0;
    for (uint8_t n : counts) {
        if (at + n > ix.size() || (at + n) * KZG355_BYTES_PER_CELL > in.size()) { std::cerr << "counts.bin asks for more than the other files hold\n"; return 2; }
        Kzg::RecoverUnit u;
        for (size_t i = at; i < at + n; i++) {
            u.first.push_back(ix[i]);
            u.second.push_back(Cell::from_bytes(&in[i * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
        }
        units.push_back(std::move(u));
        at += n;
    }
    auto r = Kzg::recover_cells_and_kzg_proofs_many_sets(units, s);
    if (r.is_err()) { std::cerr << "call error " << r.error().kind << "\n"; return 1; }
    std::ofstream out(argv[6], std::ios::binary);
    for (const auto &u : r.value()) {
        if (u.is_err()) { std::cout << "err " << u.error().kind << "\n"; continue; }
        for (const Cell &c : u.value().first) out.write(reinterpret_cast<const char *>(c.data()), KZG355_BYTES_PER_CELL);
        for (const KzgProof &p : u.value().second) out.write(reinterpret_cast<const char *>(p.data()), 48);
        std::cout << "ok\n";
    }
    return 0;
}
