// Drives Inavap::DDSolver's node selection and gap limit (include/sgufp/inavap.hpp:
// nodeSelection, gapLimit), for tests/test_frontier_select.py:
//
//   select_test <network file> <known optimum as hex float | none> <lifo | best_bound> [gap limit] [max rounds]
//
// prints "solution <value %a> <bound %a> <open> <complete> <gap %a>" and "rounds <rounds>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "sgufp/inavap.hpp"

int main(int argc, char **argv) {
    if (argc < 4 || argc > 6) {
        std::fprintf(stderr, "usage: %s <network> <known optimum hex|none> <lifo|best_bound> [gap limit] [max rounds]\n",
                     argv[0]);
        return 2;
    }
    const double known = std::strcmp(argv[2], "none") == 0 ? Inavap::DOUBLE_MIN : std::strtod(argv[2], nullptr);
    int policy;
    if (std::strcmp(argv[3], "lifo") == 0) policy = SGUFP_SELECT_LIFO;
    else if (std::strcmp(argv[3], "best_bound") == 0) policy = SGUFP_SELECT_BEST_BOUND;
    else policy = std::atoi(argv[3]);   // anything else goes to nodeSelection as a number
    try {
        auto net = std::make_shared<Network>(argv[1]);
        Inavap::DDSolver solver{net, 1};
        solver.nodeSelection(policy);
        if (argc >= 5) solver.gapLimit = std::strtod(argv[4], nullptr);
        if (argc == 6) solver.maxRounds = std::atol(argv[5]);
        const double z = solver.startSolver(known);
        std::printf("solution %a %a %lld %d %a\n", z, solver.bestBound, (long long)solver.openNodes,
                    solver.complete ? 1 : 0, solver.gap());
        std::printf("rounds %lld\n", (long long)solver.rounds);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
