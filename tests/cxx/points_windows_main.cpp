// points_windows_main.cpp -- points_windows_harness.cpp behind a main(), for a stand-alone build with -fsanitize=address,undefined
// (tests/test_points_windows_cpu.py builds and runs it; nothing is preloaded anywhere).
//
//   points_windows_main FILE format spacing stage_bytes lanes
//
// reads the stream in FILE, makes its index at `spacing` and at spacing 1 (zi_points_build), runs zpw_build for the first with the
// second as the rows to decode with, and prints "status segments batches pieces", then per segment "sum fnv1a-of-its-slot" in hex.
#include "points_windows_harness.cpp"

#include <cinttypes>

namespace {
struct rows_sink { std::vector<uint64_t> rows; void put(uint64_t bit, uint64_t pos) { rows.push_back(bit); rows.push_back(pos); } };

bool index_of(const std::vector<uint8_t>& s, uint64_t n, int format, uint64_t spacing, std::vector<uint64_t>* rows)
{
    rows_sink sink;
    std::vector<uint8_t> ring(ZI_RING);
    std::vector<zi_tables> S(1);
    std::vector<zi_sum> sum(1);
    uint64_t out_len = 0;
    if (zi_points_build(s.data(), n, format, spacing, sink, ring.data(), S[0], sum[0], &out_len) != ZI_ITEM_OK) return false;
    rows->swap(sink.rows);
    return true;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: points_windows_main FILE format spacing stage_bytes lanes\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
    fclose(f);
    const int format = atoi(argv[2]);
    const uint64_t spacing = strtoull(argv[3], nullptr, 10), stage = strtoull(argv[4], nullptr, 10);
    const uint32_t lanes = (uint32_t)strtoul(argv[5], nullptr, 10);
    const uint64_t n = s.size();
    s.push_back(0);                                            // (so that data() is no null pointer for an empty file)
    std::vector<uint64_t> rows, dense;
    if (spacing == 0 || !index_of(s, n, format, spacing, &rows) || !index_of(s, n, format, 1, &dense)) { fprintf(stderr, "no index\n"); return 2; }
    const uint64_t segments = rows.size() / 2 - 1;
    std::vector<uint8_t> windows(segments * ZI_PR_WINDOW, 0xEE);
    std::vector<uint32_t> sums(segments, 0xEEEEEEEEu);
    uint64_t stats[8];
    const int rc = zpw_build(s.data(), n, format, rows.data(), rows.size() / 2, dense.data(), dense.size() / 2, windows.data(), sums.data(),
                             nullptr, 0, stage, lanes, stats);
    if (rc == -100) { fprintf(stderr, "the harness contradicts itself\n"); return 3; }
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc, segments, stats[0], stats[5]);
    if (rc == 0) for (uint64_t k = 0; k < segments; ++k) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (uint32_t i = 0; i < ZI_PR_WINDOW; ++i) h = (h ^ windows[k * ZI_PR_WINDOW + i]) * 0x100000001b3ull;
        printf("%08" PRIx32 " %016" PRIx64 "\n", sums[k], h);
    }
    return 0;
}
