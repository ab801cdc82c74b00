// The refit's interval computation (rusterix_amd/csrc/rxr_ray_refresh.h) as a stand-alone program: tests/test_ray_refresh_cpu.py
// compares what it prints with a brute-force statement of the rule, and runs it once more under AddressSanitizer and UBSan.
//
//     ray_refresh_walk L W NTRI B0 E0 B1 E1 ...     one case on the command line
//     ray_refresh_walk L W @FILE                    a case per line of FILE: NTRI B0 E0 B1 E1 ...
//
// Per case: "case NTRI LEVELS", then per level "K COUNT DIRTY LO-HI LO-HI ...".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../rusterix_amd/csrc/rxr_ray_refresh.h"

static void run(uint32_t L, uint32_t W, const std::vector<uint32_t> &words) {
    if (words.empty()) return;
    const uint32_t ntri = words[0];
    const uint32_t n = (uint32_t)((words.size() - 1) / 2);
    const RxrRefitPlan P = rxr_refit_plan(ntri, L, W, words.data() + 1, n);
    std::printf("case %u %u\n", ntri, P.n_levels);
    for (uint32_t k = 0; k < P.n_levels; ++k) {
        std::printf("%u %u %u", k, P.cnt[k], P.dirty[k]);
        for (const RxrRefitInterval &c : P.iv[k]) std::printf(" %u-%u", c.lo, c.hi);
        std::printf("\n");
    }
}

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s L W NTRI B0 E0 ... | %s L W @FILE\n", argv[0], argv[0]);
        return 2;
    }
    const uint32_t L = (uint32_t)std::strtoul(argv[1], nullptr, 10), W = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    if (!L || !W) return 2;
    if (argv[3][0] == '@') {
        std::FILE *f = std::fopen(argv[3] + 1, "r");
        if (!f) return 2;
        std::string line;
        char buf[4096];
        while (std::fgets(buf, sizeof buf, f)) {
            line += buf;
            if (line.empty() || line.back() != '\n') continue;   // (a line longer than the buffer: keep reading)
            std::istringstream in(line);
            std::vector<uint32_t> words;
            unsigned long v;
            while (in >> v) words.push_back((uint32_t)v);
            run(L, W, words);
            line.clear();
        }
        std::fclose(f);
        return 0;
    }
    std::vector<uint32_t> words;
    for (int i = 3; i < argc; ++i) words.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    run(L, W, words);
    return 0;
}
