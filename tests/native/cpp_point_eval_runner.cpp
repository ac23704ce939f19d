// cpp_point_eval_runner -- drives the point-evaluation calls of the C++ mirror (include/kzg355.hpp) for tests/test_gpu_point_eval.py.
//   usage: cpp_point_eval_runner <trusted_setup_g1.bin> <trusted_setup_g2.bin> <cases.bin>
//   cases.bin: n inputs of 192 bytes; ALL go into one Kzg::point_evaluation_many call
//   prints one line per input: "true" | "false" | "err <kind>", then " match" | " nomatch", then the single call on the same input:
//   " <128 hex digits>" | " single_err <kind>"; one more line for an input of 191 bytes: "short <kind>"; and the versioned hash of the first
//   input's commitment: "vh <64 hex digits>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include "../../include/kzg355.hpp"

using namespace kzg355;

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::string hex(const uint8_t *p, size_t n) {
    std::string out;
    char b[3];
    for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, "%02x", p[i]); out += b; }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::cerr << "usage: cpp_point_eval_runner <g1.bin> <g2.bin> <cases.bin>\n"; return 2; }
    const std::vector<uint8_t> g1 = slurp(argv[1]), g2 = slurp(argv[2]), in = slurp(argv[3]);
    std::vector<std::vector<uint8_t>> g1v, g2v;
    for (size_t i = 0; i + 48 <= g1.size(); i += 48) g1v.emplace_back(g1.begin() + i, g1.begin() + i + 48);
    for (size_t i = 0; i + 96 <= g2.size(); i += 96) g2v.emplace_back(g2.begin() + i, g2.begin() + i + 96);
    auto rs = Kzg::load_trusted_setup(g1v, g2v);
    if (rs.is_err()) { std::cerr << "setup error " << rs.error().kind << "\n"; return 1; }
    KzgSettings s = rs.value();
    const size_t L = KZG355_BYTES_PER_POINT_EVALUATION_INPUT;
    if (in.empty() || in.size() % L) { std::cerr << "cases.bin: not a multiple of 192 bytes\n"; return 2; }
    std::vector<Kzg::PointEvaluationInput> inputs;
    for (size_t at = 0; at < in.size(); at += L) inputs.push_back(Kzg::PointEvaluationInput::from_bytes(&in[at], L).value());
    auto v = Kzg::point_evaluation_many(inputs, s);
    if (v.is_err()) { std::cout << "call err " << v.error().kind << "\n"; return 0; }
    for (size_t i = 0; i < inputs.size(); i++) {
        const Kzg::PointEvaluation &r = v.value()[i];
        if (r.result.is_err()) std::cout << "err " << r.result.error().kind;
        else std::cout << (r.result.value() ? "true" : "false");
        std::cout << (r.hash_match ? " match" : " nomatch");
        auto one = Kzg::point_evaluation(inputs[i].bytes, s);
        if (one.is_err()) std::cout << " single_err " << one.error().kind << "\n";
        else std::cout << " " << hex(one.value().data(), 64) << "\n";
    }
    auto shorter = Kzg::point_evaluation(in.data(), L - 1, s);
    std::cout << "short " << (shorter.is_err() ? (int)shorter.error().kind : -1) << "\n";
    auto h = Kzg::kzg_to_versioned_hash(KzgCommitment::from_bytes(&in[96], 48).value());
    std::cout << "vh " << (h.is_ok() ? hex(h.value().data(), 32) : std::string("err")) << "\n";
    return 0;
}
