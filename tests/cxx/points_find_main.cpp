// points_find_main.cpp -- points_find_harness.cpp behind a main(), for a stand-alone build with -fsanitize=address,undefined
// (tests/test_points_find_cpu.py builds and runs it; nothing is preloaded anywhere).
//
//   points_find_main FILE format chunk_bytes spacing limit_bytes
//
// reads the stream in FILE, runs zpf_index with one lane and prints "status entries out_len candidates dropped rounds jobs",
// then one row "in_bit out_byte" per line.
#include "points_find_harness.cpp"

#include <cinttypes>

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: points_find_main FILE format chunk_bytes spacing limit_bytes\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    const int format = atoi(argv[2]);
    const uint64_t chunk = strtoull(argv[3], nullptr, 10), spacing = strtoull(argv[4], nullptr, 10), slack = strtoull(argv[5], nullptr, 10);
    if (chunk < 16) { fprintf(stderr, "chunk_bytes must be at least 16\n"); return 2; }
    const uint64_t cap = s.size() / chunk + 3;
    std::vector<uint64_t> rows(2 * cap);
    uint64_t entries = 0, out_len = 0, stats[4] = { 0, 0, 0, 0 };
    s.push_back(0);                                            // (so that data() is no null pointer for an empty file)
    const int rc = zpf_index(s.data(), s.size() - 1, format, chunk, spacing, slack, 1, rows.data(), cap, &entries, &out_len, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc, entries, out_len, stats[0], stats[1], stats[2], stats[3]);
    if (rc == 0) for (uint64_t i = 0; i < entries; ++i) printf("%" PRIu64 " %" PRIu64 "\n", rows[2 * i], rows[2 * i + 1]);
    return 0;
}
