// cpp_cell_recover_at_runner -- drives Kzg::recover_cells_and_kzg_proofs_at and Kzg::recover_cells_and_kzg_proofs_at_many_sets of the C++
// mirror (include/kzg355.hpp) for tests/test_gpu_cell_recover_at.py.
//   usage: cpp_cell_recover_at_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <counts.bin> <indices.bin> <cells.bin> <want_counts.bin>
//          <want_indices.bin> <out.bin> [single]
//   counts.bin: the number of known cells per unit, one byte each; indices.bin: the units' known cell indices back to back, one byte each;
//   cells.bin: the known cells (2048 bytes each) in the same order; want_counts.bin / want_indices.bin: the same two lists for the wanted
//   cells.  "single": one recover_cells_and_kzg_proofs_at call per unit instead of one _many_sets call.
//   out.bin: per computed unit its wanted cells (2048 bytes each) then their proofs (48 bytes each); prints one line per unit: "ok" | "err <kind>"
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
    if (argc < 9) {
        std::cerr << "usage: cpp_cell_recover_at_runner <g1.bin> <g2.bin> <counts.bin> <indices.bin> <cells.bin> <want_counts.bin> <want_indices.bin> "
                     "<out.bin> [single]\n";
        return 2;
    }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), counts = slurp(argv[3]), ix = slurp(argv[4]), in = slurp(argv[5]),
                               wcounts = slurp(argv[6]), wix = slurp(argv[7]);
    const bool single = argc > 9 && !std::strcmp(argv[9], "single");
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    if (wcounts.size() != counts.size() || ix.size() * KZG355_BYTES_PER_CELL != in.size()) { std::cerr << "the input files disagree\n"; return 2; }
    std::vector<Kzg::RecoverAtUnit> units;
    size_t at = 0, wat = 0;
    for (size_t u = 0; u < counts.size(); u++) {
        if (at + counts[u] > ix.size() || wat + wcounts[u] > wix.size()) { std::cerr << "the counts ask for more than the index files hold\n"; return 2; }
        Kzg::RecoverAtUnit unit;
        unit.cell_indices.assign(ix.begin() + at, ix.begin() + at + counts[u]);
        for (size_t j = at; j < at + counts[u]; j++) unit.cells.push_back(Cell::from_bytes(&in[j * KZG355_BYTES_PER_CELL], KZG355_BYTES_PER_CELL).value());
        unit.want_indices.assign(wix.begin() + wat, wix.begin() + wat + wcounts[u]);
        units.push_back(std::move(unit));
        at += counts[u];
        wat += wcounts[u];
    }
    std::vector<Result<std::pair<std::vector<Cell>, std::vector<KzgProof>>>> res;
    if (single) for (const auto &u : units) res.push_back(Kzg::recover_cells_and_kzg_proofs_at(u.cell_indices, u.cells, u.want_indices, s));
    else {
        auto r = Kzg::recover_cells_and_kzg_proofs_at_many_sets(units, s);
        if (r.is_err()) { std::cerr << "call error " << r.error().kind << "\n"; return 1; }
        res = r.value();
    }
    std::ofstream out(argv[8], std::ios::binary);
    for (const auto &u : res) {
        if (u.is_err()) { std::cout << "err " << u.error().kind << "\n"; continue; }
        for (const Cell &c : u.value().first) out.write(reinterpret_cast<const char *>(c.data()), KZG355_BYTES_PER_CELL);
        for (const KzgProof &p : u.value().second) out.write(reinterpret_cast<const char *>(p.data()), 48);
        std::cout << "ok\n";
    }
    return 0;
}
