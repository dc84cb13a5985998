// members_points_decode_main.cpp -- members_points_decode_harness.cpp behind a main(), for a stand-alone build with
// -fsanitize=address,undefined (tests/test_members_points_decode_cpu.py builds and runs it; nothing is preloaded anywhere).
//
//   members_points_decode_main FILE ROWS batch_bytes cap
//
// reads the file and its rows (ROWS: one "in_bit out_byte" per line, in_bit hexadecimal, as members_points_main prints them), runs
// zmpd_decode with one lane into exactly `cap` bytes and prints
//   "decode status out_len crc32 members proven segments batches pending rounds serial turns"
// (crc32 over the decoded bytes, 0 unless the status is 0).
#include "members_points_decode_harness.cpp"

#include <cinttypes>

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: members_points_decode_main FILE ROWS batch_bytes cap\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    FILE* r = fopen(argv[2], "r");
    if (!r) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<uint64_t> rows;
    uint64_t bit, pos;
    while (fscanf(r, "%" SCNx64 " %" SCNu64, &bit, &pos) == 2) { rows.push_back(bit); rows.push_back(pos); }
    fclose(r);
    const uint64_t batch = strtoull(argv[3], nullptr, 10), cap = strtoull(argv[4], nullptr, 10);
    const uint64_t n = s.size(), entries = rows.size() / 2;
    s.push_back(0);                                            // (so that data() is no null pointer for an empty file)
    rows.push_back(0);
    std::vector<uint8_t> out(cap);                             // exactly cap bytes: the address sanitizer sees a write behind them
    uint64_t out_len = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const int rc = zmpd_decode(s.data(), n, rows.data(), entries, out.data(), cap, batch, 1, &out_len, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    uint32_t c = 0;
    if (rc == 0) {
        c = ~0u;
        for (uint64_t i = 0; i < out_len; ++i) { c ^= out[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * 0xEDB88320u); }
        c = ~c;
    }
    printf("decode %d %" PRIu64 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc,
           rc == 0 ? out_len : 0, c, stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], stats[7]);
    return 0;
}
