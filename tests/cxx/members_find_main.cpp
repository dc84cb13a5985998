// members_find_main.cpp -- members_find_harness.cpp behind a main(), for a stand-alone build with -fsanitize=address,undefined
// (tests/test_members_find_cpu.py builds and runs it; nothing is preloaded anywhere).
//
//   members_find_main FILE limit_bytes cap
//
// reads the file, runs zmf_find and zmf_decode with one lane and prints
//   "find status entries members candidates dropped rounds jobs", one row "file_offset decoded_offset" per line, then
//   "decode status out_len crc32" (out_len and the CRC-32 of the decoded bytes: 0 0 unless status is 0).
#include "members_find_harness.cpp"

#include <cinttypes>

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: members_find_main FILE limit_bytes cap\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    const uint64_t limit = strtoull(argv[2], nullptr, 10), cap = strtoull(argv[3], nullptr, 10);
    if (limit == 0) { fprintf(stderr, "limit_bytes must be at least 1\n"); return 2; }
    const uint64_t n = s.size(), max_entries = n / 20 + 2;
    s.push_back(0);                                            // (so that data() is no null pointer for an empty file)
    std::vector<uint64_t> rows(2 * max_entries);
    uint64_t entries = 0, stats[5] = { 0, 0, 0, 0, 0 };
    int rc = zmf_find(s.data(), n, limit, 1, rows.data(), max_entries, &entries, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    printf("find %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc, entries, stats[0], stats[1], stats[2], stats[3], stats[4]);
    if (rc == 0) for (uint64_t i = 0; i < entries; ++i) printf("%" PRIu64 " %" PRIu64 "\n", rows[2 * i], rows[2 * i + 1]);
    std::vector<uint8_t> out(cap + 1);
    uint64_t out_len = 0;
    rc = zmf_decode(s.data(), n, out.data(), cap, limit, 1, &out_len, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    uint32_t c = 0;
    if (rc == 0) {
        c = ~0u;
        for (uint64_t i = 0; i < out_len; ++i) { c ^= out[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) * 0xEDB88320u); }
        c = ~c;
    }
    printf("decode %d %" PRIu64 " %" PRIu32 "\n", rc, rc == 0 ? out_len : 0, c);
    return 0;
}
