// point_eval_probe.cpp -- host build of the point-evaluation precompile's byte layout (kzg_rust_amd/csrc/point_eval.h), the function k_pe_unpack
// runs per lane, here with sha256_block of sha256.h as the compression.  A stand-alone program for tests/test_point_eval_abi.py, which builds it
// plain and with -fsanitize=address,undefined:
//   point_eval_probe <file of n * 192 bytes>   prints per input "<match> <record, 320 hex digits> <versioned hash of the commitment, 64 hex digits>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kzg_rust_amd/csrc/point_eval.h"

using namespace kzg;

static void put_hex(const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", p[i]); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
    fclose(f);
    if (data.size() % PE_INPUT_BYTES) { fprintf(stderr, "%zu bytes: not a multiple of %d\n", data.size(), PE_INPUT_BYTES); return 2; }
    for (size_t i = 0; i < data.size() / PE_INPUT_BYTES; i++) {
        uint32_t in[PE_INPUT_WORDS], rec[PE_RECORD_WORDS], vh[PE_HASH_WORDS];
        memcpy(in, data.data() + PE_INPUT_BYTES * i, PE_INPUT_BYTES);
        const uint32_t m = pe_unpack(rec, in, PeHostCompress());
        pe_versioned_hash(vh, in + PE_IN_C, PeHostCompress());
        uint8_t out[4 * PE_RECORD_WORDS], h[4 * PE_HASH_WORDS];
        memcpy(out, rec, sizeof out);
        memcpy(h, vh, sizeof h);
        printf("%u ", m); put_hex(out, sizeof out); printf(" "); put_hex(h, sizeof h); printf("\n");
    }
    return 0;
}
