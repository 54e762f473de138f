// commit_host.cpp -- bk_bn256.h on the host, stand-alone.
//
//   commit_host run FILE          one command per line, one result line each
//       fmul A B | fadd A B | fsub A B | finv A      field elements, 64 hex digits
//       padd P Q | pdbl P | smul V P | rt P          points, 128 hex digits; V decimal int64
//       msm N V.. P..                                sum V_i P_i, windowed
//     a point that does not unmarshal prints "bad"
//   commit_host bench N THREADS ALGO REPS
//       the time of sum v_i PK_i, PK_i = 2^i G, v_i a fixed signed sequence:
//       ALGO 0 plain double-and-add on the reduced scalar (254 bits for v < 0),
//       1 double-and-add on |v|, 2 the signed 4-bit windows over the key's
//       table (built outside the timed part).  Prints the best of REPS in ms.
//
// tests/test_commit_host.py builds and runs it (plainly, and with the address
// and undefined-behaviour sanitizers); tools/commit_bench.py uses bench.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "bk_bn256.h"

using namespace bk::bn;

static bool hex_bytes(const std::string &s, uint8_t *out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; ++i) {
        unsigned v;
        if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

static std::string bytes_hex(const uint8_t *b, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s.push_back(d[b[i] >> 4]);
        s.push_back(d[b[i] & 15]);
    }
    return s;
}

static bool read_fp(std::istream &in, Fp *a) {
    std::string s;
    uint8_t b[32];
    if (!(in >> s) || !hex_bytes(s, b, 32)) return false;
    *a = fp_to_mont(fp_from_bytes(b));
    return true;
}

static std::string show_fp(const Fp &a) {
    uint8_t b[32];
    fp_to_bytes(fp_from_mont(a), b);
    return bytes_hex(b, 32);
}

static bool read_pt(std::istream &in, Aff *a) {
    std::string s;
    uint8_t b[64];
    if (!(in >> s) || !hex_bytes(s, b, 64)) return false;
    return aff_unmarshal(b, a);
}

static std::string show_pt(const Jac &a) {
    uint8_t b[64];
    aff_marshal(jac_to_aff(a), b);
    return bytes_hex(b, 64);
}

// the table of p: k p for k = 1 .. TABLE
static void build_table(const Aff &p, Aff *t) {
    Jac a = jac_from_aff(p);
    t[0] = p;
    for (int k = 1; k < TABLE; ++k) {
        a = jac_add_aff(a, p);
        t[k] = jac_to_aff(a);
    }
}

// sum v_i P_i over i = first, first + step, ...: the windows share their doublings
static Jac msm_windows(const int64_t *v, const Aff *tables, size_t n, size_t first, size_t step) {
    Jac acc = jac_inf();
    for (int w = WINDOWS - 1; w >= 0; --w) {
        if (w != WINDOWS - 1)
            for (int k = 0; k < 4; ++k) acc = jac_dbl(acc);
        for (size_t i = first; i < n; i += step) {
            int dg = scalar_digit(scalar_abs(v[i]), w);
            if (dg == 0) continue;
            if (v[i] < 0) dg = -dg;
            const Aff &e = tables[i * TABLE + (size_t)(dg < 0 ? -dg : dg) - 1];
            acc = jac_add_aff(acc, dg < 0 ? aff_neg(e) : e);
        }
    }
    return acc;
}

// v P the way the reference multiplies: double-and-add over all the bits of v
// mod n (n - |v| for v < 0)
static Jac mul_reduced(const Aff &p, int64_t v) {
    static const uint32_t ORDER[8] = {0x57ac7261u, 0x1a2ef45bu, 0xf82b3924u, 0x2e8d8e12u,
                                      0x6184dc21u, 0xaa6fecb8u, 0x4aa387f9u, 0x8fb501e3u};
    uint32_t s[8] = {0};
    const uint64_t m = scalar_abs(v);
    s[0] = (uint32_t)m;
    s[1] = (uint32_t)(m >> 32);
    if (v < 0) {
        uint64_t br = 0;
        for (int i = 0; i < 8; ++i) {
            const uint64_t t = (uint64_t)ORDER[i] - s[i] - br;
            s[i] = (uint32_t)t;
            br = t >> 63;
        }
    }
    Jac r = jac_inf();
    for (int bit = 255; bit >= 0; --bit) {
        r = jac_dbl(r);
        if ((s[bit >> 5] >> (bit & 31)) & 1u) r = jac_add_aff(r, p);
    }
    return r;
}

static int run(const char *path) {
    std::ifstream f(path);
    if (!f) return 2;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        Fp a, b;
        Aff p, q;
        if (op == "fmul" || op == "fadd" || op == "fsub") {
            if (!read_fp(in, &a) || !read_fp(in, &b)) return 3;
            const Fp r = op == "fmul" ? fp_mul(a, b) : op == "fadd" ? fp_add(a, b) : fp_sub(a, b);
            std::cout << show_fp(r) << "\n";
        } else if (op == "finv") {
            if (!read_fp(in, &a)) return 3;
            std::cout << show_fp(fp_inv(a)) << "\n";
        } else if (op == "padd") {
            const bool ok1 = read_pt(in, &p), ok2 = read_pt(in, &q);
            if (!ok1 || !ok2) {
                std::cout << "bad\n";
                continue;
            }
            // once as a mixed and once as a general addition: they must agree
            const std::string m = show_pt(jac_add_aff(jac_from_aff(p), q));
            // a general addition of operands with z != 1
            const Jac p2 = jac_add(jac_dbl(jac_from_aff(p)), jac_from_aff(aff_neg(p)));
            const Jac q2 = jac_add(jac_dbl(jac_from_aff(q)), jac_from_aff(aff_neg(q)));
            const std::string g = show_pt(jac_add(p2, q2));
            std::cout << (m == g ? m : "mismatch " + m + " " + g) << "\n";
        } else if (op == "pdbl") {
            if (!read_pt(in, &p)) {
                std::cout << "bad\n";
                continue;
            }
            std::cout << show_pt(jac_dbl(jac_from_aff(p))) << "\n";
        } else if (op == "smul") {
            long long v;
            if (!(in >> v)) return 3;
            if (!read_pt(in, &p)) {
                std::cout << "bad\n";
                continue;
            }
            const std::string s1 = show_pt(jac_mul_i64(p, v));
            const std::string s2 = show_pt(mul_reduced(p, v));
            Aff t[TABLE];
            build_table(p, t);
            const int64_t vv = v;
            const std::string s3 = show_pt(msm_windows(&vv, t, 1, 0, 1));
            std::cout << (s1 == s2 && s1 == s3 ? s1 : "mismatch " + s1 + " " + s2 + " " + s3) << "\n";
        } else if (op == "rt") {
            if (!read_pt(in, &p)) {
                std::cout << "bad\n";
                continue;
            }
            std::cout << show_pt(jac_from_aff(p)) << "\n";
        } else if (op == "msm") {
            size_t n;
            if (!(in >> n) || n > 4096) return 3;
            std::vector<int64_t> v(n);
            std::vector<Aff> t(n * TABLE);
            for (size_t i = 0; i < n; ++i) {
                long long x;
                if (!(in >> x)) return 3;
                v[i] = x;
            }
            bool ok = true;
            for (size_t i = 0; i < n; ++i) {
                if (!read_pt(in, &p)) {
                    ok = false;
                    break;
                }
                build_table(p, &t[i * TABLE]);
            }
            if (!ok) {
                std::cout << "bad\n";
                continue;
            }
            std::cout << show_pt(msm_windows(v.data(), t.data(), n, 0, 1)) << "\n";
        } else {
            return 4;
        }
    }
    return 0;
}

static int bench(size_t n, int threads, int algo, int reps) {
    if (n < 1 || threads < 1 || threads > 256 || algo < 0 || algo > 2 || reps < 1) return 2;
    std::vector<Aff> key(n), tables;
    std::vector<int64_t> v(n);
    Jac g = Jac{fp_one(), fp_neg(fp_dbl(fp_one())), fp_one()};
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < n; ++i) {
        key[i] = jac_to_aff(g);
        g = jac_dbl(g);
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        // magnitudes of a quantised update (about 2^20), both signs
        v[i] = (int64_t)((x >> 43) & 0xfffff) * ((x >> 63) ? -1 : 1);
    }
    if (algo == 2) {
        tables.resize(n * TABLE);
        for (size_t i = 0; i < n; ++i) build_table(key[i], &tables[i * TABLE]);
    }
    double best = 1e300;
    std::string shown;
    for (int r = 0; r < reps; ++r) {
        std::vector<Jac> part((size_t)threads, jac_inf());
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                Jac acc = jac_inf();
                if (algo == 2) {
                    acc = msm_windows(v.data(), tables.data(), n, (size_t)t, (size_t)threads);
                } else {
                    for (size_t i = (size_t)t; i < n; i += (size_t)threads)
                        acc = jac_add(acc, algo == 0 ? mul_reduced(key[i], v[i])
                                                     : jac_mul_i64(key[i], v[i]));
                }
                part[(size_t)t] = acc;
            });
        for (auto &th : pool) th.join();
        Jac acc = jac_inf();
        for (int t = 0; t < threads; ++t) acc = jac_add(acc, part[(size_t)t]);
        shown = show_pt(acc);
        const double ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best) best = ms;
    }
    printf("%.6f %s\n", best, shown.c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
    if (argc == 6 && !strcmp(argv[1], "bench"))
        return bench((size_t)atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    fprintf(stderr, "usage: commit_host run FILE | bench N THREADS ALGO REPS\n");
    return 1;
}
