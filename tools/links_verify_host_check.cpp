// Stand-alone host check of the per-lane body of k_links_verify (sarlacc_amd/csrc/links_verify_core.hpp, DESIGN §4.19 rule
// 6a) against a plain banded DP with infinite cells outside the band: 60 000 random pairs (noisy copies and unrelated
// reads, with bytes that are no base, lengths 0 .. 300, either strand), every bandwidth class in every word count that
// holds it, once without a bound and once with a random one.  The reads are heap blocks of their exact size, so the
// host's sanitizers see any byte read outside a read:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Isarlacc_amd/csrc \
//         tools/links_verify_host_check.cpp -o /tmp/links_verify_host_check && /tmp/links_verify_host_check
#include "links_verify_core.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace sarlacc;

static bool match(uint8_t a, uint8_t b) { return a == b && (a == 'A' || a == 'C' || a == 'G' || a == 'T'); }

static std::string rc(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (auto& c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
    return r;
}

static long long naive(const std::string& x, const std::string& y, int w) {
    const long long INF = 1LL << 40;
    const int lx = x.size(), ly = y.size();
    if (std::abs(lx - ly) > w) return INF;
    std::vector<std::vector<long long>> D(lx + 1, std::vector<long long>(ly + 1, INF));
    for (int i = 0; i <= lx; ++i)
        for (int j = 0; j <= ly; ++j) {
            if (std::abs(i - j) > w) continue;
            if (i == 0 && j == 0) { D[i][j] = 0; continue; }
            long long v = INF;
            if (i > 0 && j > 0) v = std::min(v, D[i - 1][j - 1] + (match(x[i - 1], y[j - 1]) ? 0 : 1));
            if (i > 0) v = std::min(v, D[i - 1][j] + 1);
            if (j > 0) v = std::min(v, D[i][j - 1] + 1);
            D[i][j] = v;
        }
    return D[lx][ly];
}

template <int NW>
static int run(const std::string& x, const std::string& y, int w, bool rev, int limit) {
    // exact-size heap copies: the sanitizer sees any byte read outside the read
    std::vector<uint8_t> a(x.begin(), x.end()), b(y.begin(), y.end());
    uint8_t* pa = static_cast<uint8_t*>(malloc(a.size() ? a.size() : 1));
    uint8_t* pb = static_cast<uint8_t*>(malloc(b.size() ? b.size() : 1));
    std::copy(a.begin(), a.end(), pa);
    std::copy(b.begin(), b.end(), pb);
    // an empty read points at the end of its one-byte block
    const int r = lv_banded<NW>(a.empty() ? pa + 1 : pa, x.size(), b.empty() ? pb + 1 : pb, y.size(), w, rev, limit);
    free(pa);
    free(pb);
    return r;
}

int main() {
    std::mt19937_64 rng(12345);
    const char alpha[] = "ACGTACGTACGTACGTNa";
    long long checked = 0, bad = 0;
    const int ws[] = {0, 1, 2, 3, 8, 15, 16, 31, 32, 63, 64, 100, 111, 112, 127};
    for (int it = 0; it < 60000; ++it) {
        const int w = ws[rng() % 15];
        const int maxlen = (it % 7 == 0) ? 300 : 40;
        int lx = rng() % (maxlen + 1);
        int dl = static_cast<int>(rng() % (2 * std::min(w, 12) + 1)) - std::min(w, 12);
        if (rng() % 5 == 0) dl = (rng() & 1) ? w : -w;
        int ly = std::max(0, lx + dl);
        if (std::abs(lx - ly) > w) continue;
        std::string x(lx, 'A'), y;
        const int na = (rng() % 4 == 0) ? 4 : 18;      // pure ACGT or with non-bases
        for (auto& c : x) c = alpha[rng() % na];
        if (rng() % 2) {      // y a noisy copy of x
            for (int i = 0; i < lx; ++i) {
                const int r = rng() % 20;
                if (r == 0) continue;
                if (r == 1) y += alpha[rng() % na];
                y += r == 2 ? alpha[rng() % na] : x[i];
            }
            y.resize(ly, 'C');
        } else {
            y.assign(ly, 'A');
            for (auto& c : y) c = alpha[rng() % na];
        }
        const bool rev = rng() & 1;
        const std::string yy = rev ? rc(y) : y;      // the kernel sees yy and undoes it with rev
        const long long want = naive(x, rev ? rc(yy) : yy, w);
        const int limits[2] = {1 << 30, static_cast<int>(rng() % (std::max(lx, ly) + 1))};
        for (int L = 0; L < 2; ++L) {
            const int limit = limits[L];
            int got[5] = {-1, -1, -1, -1, -1};
            if (2 * w + 1 <= 32) got[0] = run<1>(x, yy, w, rev, limit);
            if (2 * w + 1 <= 64) got[1] = run<2>(x, yy, w, rev, limit);
            if (2 * w + 1 <= 128) got[2] = run<4>(x, yy, w, rev, limit);
            if (2 * w + 1 <= 224) got[3] = run<7>(x, yy, w, rev, limit);
            got[4] = run<8>(x, yy, w, rev, limit);
            for (int g = 0; g < 5; ++g) {
                if (got[g] < 0) continue;
                ++checked;
                const bool ok = want <= limit ? got[g] == want : got[g] > limit;
                if (!ok && ++bad < 20)
                    printf("BAD w %d NW# %d rev %d limit %d want %lld got %d\n x %s\n y %s\n", w, g, rev, limit, want, got[g], x.c_str(), yy.c_str());
            }
        }
    }
    printf("checked %lld bad %lld\n", checked, bad);
    return bad != 0;
}
