// members_points_main.cpp -- members_points_harness.cpp behind a main(), for a stand-alone build with -fsanitize=address,undefined
// (tests/test_members_points_cpu.py builds and runs it; nothing is preloaded anywhere).
//
//   members_points_main FILE chunk_bytes own_limit
//
// reads the file, runs zmp_index with one lane and prints
//   "index status entries out_len members header_candidates block_candidates dropped rounds jobs", one row "in_bit out_byte"
//   per line (hexadecimal in_bit), then "index_pairs n" (zmp_to_index's count over the rows: members + 1, or 0).
#include "members_points_harness.cpp"

#include <cinttypes>

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: members_points_main FILE chunk_bytes own_limit\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    const uint64_t chunk = strtoull(argv[2], nullptr, 10), own = strtoull(argv[3], nullptr, 10);
    if (chunk < 16) { fprintf(stderr, "chunk_bytes must be at least 16\n"); return 2; }
    const uint64_t n = s.size(), max_entries = n / 10 + n / chunk + 4;
    s.push_back(0);                                            // (so that data() is no null pointer for an empty file)
    std::vector<uint64_t> rows(2 * max_entries);
    uint64_t entries = 0, total = 0, stats[6] = { 0, 0, 0, 0, 0, 0 };
    int rc = zmp_index(s.data(), n, chunk, 1, own, 1, rows.data(), max_entries, &entries, &total, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    printf("index %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc, entries, total,
           stats[0], stats[1], stats[2], stats[3], stats[4], stats[5]);
    if (rc == 0) for (uint64_t i = 0; i < entries; ++i) printf("%" PRIx64 " %" PRIu64 "\n", rows[2 * i], rows[2 * i + 1]);
    std::vector<uint64_t> pairs(2 * (entries + 1));
    printf("index_pairs %" PRIu64 "\n", rc == 0 ? zmp_to_index(rows.data(), entries, pairs.data(), entries + 1) : 0);
    return 0;
}
