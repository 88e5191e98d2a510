// Host check of the solo K4 kernel's barrier schedule (nnest_amd/csrc/solo_schedule.h), built and run by tests/test_solo_schedule.py.
// Each role's loops are restated here with the bounds the kernel takes from the header, as a list of the barriers it arrives at; the
// lists must be the same barrier for barrier (a role that has ended is excused from the rest), and as long as the header's counts say.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "solo_schedule.h"

using namespace nnest;

enum { P = 1 << 20, A = 2 << 20, B = 3 << 20, F = 4 << 20 };   // barrier kinds, | the step or buffer they belong to

static std::vector<int> net_wave(int S, int warm, bool exact_all) {
    std::vector<int> b;
    b.push_back(P | 0);                                  // fetch_noise(0)
    if (warm > 0) {
        b.push_back(P | 1);                              // step 1's fetch
        for (int it = 1; it <= warm; ++it) {
            b.push_back(A | it);
            b.push_back(P | (it + 1));
            b.push_back(B | it);
        }
    }
    int it = solo_first_straight_step(warm);
    if (it <= S && (it & 1)) { b.push_back(P | it); ++it; }
    for (; it < S; it += 2) { b.push_back(P | it); b.push_back(P | (it + 1)); }
    if (it <= S) b.push_back(P | it);
    if (exact_all) b.push_back(F);
    return b;
}

static std::vector<int> noise_wave(int S, int warm) {
    std::vector<int> b;
    b.push_back(P | 0);
    if (S >= 1) {
        b.push_back(P | 1);
        for (int k = 1; k <= warm; ++k) {
            b.push_back(A | k);
            b.push_back(P | (k + 1));
            b.push_back(B | k);
        }
        for (int k = solo_first_lagged_fetch(warm); k <= S; ++k) b.push_back(P | k);
    }
    return b;
}

static std::vector<int> relay_wave(int S, int warm, bool dynamic, bool exact_all) {
    std::vector<int> b;
    if (!dynamic) return b;
    const int k0 = solo_relay_first_iteration(warm);
    if (warm > 0) {
        b.push_back(P | 0);
        b.push_back(P | 1);
        for (int k = 1; k <= warm; ++k) {
            b.push_back(A | k);
            b.push_back(P | (k + 1));
            b.push_back(B | k);
        }
    }
    for (int k2 = k0; k2 <= S; k2 += 2) {
        b.push_back(P | k2);
        if (k2 + 1 <= S) b.push_back(P | (k2 + 1));
    }
    if (exact_all) b.push_back(F);
    return b;
}

static int fails = 0;
#define CHECK(c)                                                                                                      \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            ++fails;                                                                                                  \
            std::printf("FAIL %s  (S %d, warm flag %d -> %d, dynamic %d, exact_all %d)\n", #c, S, flag, warm, (int)dynamic, (int)exact_all); \
        }                                                                                                             \
    } while (0)

int main() {
    int cases = 0;
    for (int S = 1; S <= 40; ++S) {
        const int flags[5] = {0, 1, 16, S - 1, S};
        for (int f = 0; f < 5; ++f)
            for (int rule = 0; rule < 3; ++rule) {
                const int flag = flags[f];
                const bool dynamic = rule != 0, exact_all = rule == 2;
                const int warm = solo_warm_steps(S, flag, dynamic, exact_all);
                ++cases;
                CHECK(warm >= 0 && warm <= S - 1);
                CHECK(dynamic || warm == 0);
                CHECK(!exact_all || warm == S - 1);
                const std::vector<int> net = net_wave(S, warm, exact_all), noise = noise_wave(S, warm), relay = relay_wave(S, warm, dynamic, exact_all);
                // the header's counts are the loops' counts
                CHECK((int)net.size() == solo_net_barriers(S, warm, dynamic, exact_all));
                CHECK((int)noise.size() == solo_noise_barriers(S, warm, dynamic, exact_all));
                CHECK((int)relay.size() == solo_relay_barriers(S, warm, dynamic, exact_all));
                // ... and what the net waves need of the other two roles
                CHECK((int)noise.size() == solo_noise_barriers_due(S, warm, dynamic, exact_all));
                CHECK((int)relay.size() == solo_relay_barriers_due(S, warm, dynamic, exact_all));
                if (dynamic && !exact_all) CHECK(net.size() == noise.size() && net.size() == relay.size());
                // the same barrier at the same place (the noise wave ends in front of F; without the rule the relay has ended)
                bool same = true;
                for (size_t i = 0; i < noise.size() && i < net.size(); ++i) same = same && noise[i] == net[i];
                for (size_t i = 0; i < relay.size() && i < net.size(); ++i) same = same && relay[i] == net[i];
                CHECK(same);
                CHECK(noise.size() + (exact_all ? 1 : 0) == net.size());
                // every step's buffer is fetched exactly once, in order: P0, then P_1 .. P_S
                int next = 0;
                for (int v : net)
                    if ((v >> 20) == (P >> 20)) { CHECK((v & 0xfffff) == next); ++next; }
                CHECK(next == S + 1);
                // lag 0 never enters the straight loop (beyond a launch of one step, which has no exact step at all)
                if (exact_all && S > 1) CHECK(solo_first_straight_step(warm) > S);
            }
    }
    std::printf("%d cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
