// check_apply_route.cpp -- apply_route (csrc/kmg_apply_route.h) against the recorded decisions of apply_route_table.txt: one line
// per (mode, k, forced, mask_words) with pairs (n_pixels_hint, route) behind it.  The table was written once by the rule as it stood
// inside plan_create before it became a function.  Stops at the first difference.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "kmg_apply_route.h"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: check_apply_route apply_route_table.txt\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char line[1 << 16];
    unsigned long rows = 0, points = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int mode, forced, mask_words, used = 0;
        uint32_t k;
        if (sscanf(line, "%d %" SCNu32 " %d %d%n", &mode, &k, &forced, &mask_words, &used) != 4) { fprintf(stderr, "bad line: %s", line); return 2; }
        ++rows;
        const char *s = line + used;
        uint64_t n;
        int want, step;
        while (sscanf(s, " %" SCNu64 " %d%n", &n, &want, &step) == 2) {
            s += step;
            ++points;
            const int got = (int)kmg::apply_route(mode, k, n, forced, mask_words != 0);
            if (got != want) {
                printf("mode %d k %" PRIu32 " n %" PRIu64 " forced %d mask_words %d: route %d, recorded %d\n", mode, k, n, forced, mask_words, got, want);
                return 1;
            }
        }
    }
    fclose(f);
    printf("rows %lu points %lu route_mismatches 0\n", rows, points);
    return rows == 4 * 11 * 3 * 2 ? 0 : 1;
}
