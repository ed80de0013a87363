// Drives what Inavap::DDSolver leaves besides its value (include/sgufp/inavap.hpp: bestPath,
// bestBound, openNodes, gap; GuroSolver::solveFlows), for tests/test_solution_host.py:
//
//   solution_test <network file> <known optimum as hex float | none> [max rounds]
//
// prints "solution <value %a> <bound %a> <open> <complete> <gap %a>", "path <len> <decisions>"
// and, when a routing is known, one "flows <scenario> <status> <sum of the arc flows>" line per
// scenario (GuroSolver::solveFlows on that path).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "sgufp/inavap.hpp"

int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: %s <network> <known optimum hex|none> [max rounds]\n", argv[0]);
        return 2;
    }
    const double known = std::strcmp(argv[2], "none") == 0 ? Inavap::DOUBLE_MIN : std::strtod(argv[2], nullptr);
    try {
        auto net = std::make_shared<Network>(argv[1]);
        Inavap::DDSolver solver{net, 1};
        if (argc == 4) solver.maxRounds = std::atol(argv[3]);
        const double z = solver.startSolver(known);
        std::printf("solution %a %a %lld %d %a\n", z, solver.bestBound, (long long)solver.openNodes,
                    solver.complete ? 1 : 0, solver.gap());
        std::printf("path %zu", solver.bestPath.size());
        for (auto d : solver.bestPath) std::printf(" %d", (int)d);
        std::printf("\n");
        if (!solver.bestPath.empty()) {
            Inavap::GuroSolver sub{net};
            std::vector<int32_t> status;
            const auto flows = sub.solveFlows(solver.bestPath, &status);
            for (size_t s = 0; s < flows.size(); s++) {
                long long sum = 0;
                for (auto x : flows[s]) sum += x;
                std::printf("flows %zu %d %lld\n", s, (int)status[s], sum);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
