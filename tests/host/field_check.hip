// TEST INFRASTRUCTURE -- host check of csrc/field.hpp (tests/test_field_host.py).
// The host pass of hipcc compiles the MH_HD functions of field.hpp; this
// stand-alone program applies them to every ordered pair of the values it reads
// and prints the results for the test to compare with Python integers.  Built
// with -fsanitize=undefined, so an overflowing shift or signed overflow in the
// __int128 arithmetic aborts the run.
//
//   field_check <64|128> < values        (one hexadecimal value per line, each < 2^64 / 2^128)
// prints, for every ordered pair (a, b):  a b add sub mul neg(a) inv(a)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "field.hpp"

static mh_u128 parse_hex(const char* s) {
    mh_u128 v = 0;
    for (; *s; s++) {
        int d;
        if (*s >= '0' && *s <= '9') d = *s - '0';
        else if (*s >= 'a' && *s <= 'f') d = *s - 'a' + 10;
        else break;
        v = (v << 4) | (unsigned)d;
    }
    return v;
}

static F64::E make(F64*, mh_u128 v) { return (uint64_t)v; }
static F128::E make(F128*, mh_u128 v) { return F128::E{(uint64_t)v, (uint64_t)(v >> 64)}; }
static void put(F64::E x) { printf("%016llx", (unsigned long long)x); }
static void put(F128::E x) { printf("%016llx%016llx", (unsigned long long)x.hi, (unsigned long long)x.lo); }

template <class F>
static int run() {
    typedef typename F::E E;
    std::vector<E> vals;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n' || line[0] == 0) continue;
        vals.push_back(make((F*)nullptr, parse_hex(line)));
    }
    for (const E& a : vals) {
        if (!F::valid(a)) {
            fprintf(stderr, "field_check: value out of range\n");
            return 2;
        }
    }
    for (const E& a : vals) {
        const E na = F::neg(a), ia = finv<F>(a);
        for (const E& b : vals) {
            const E r[7] = {a, b, F::add(a, b), F::sub(a, b), F::mul(a, b), na, ia};
            for (int i = 0; i < 7; i++) {
                put(r[i]);
                putchar(i == 6 ? '\n' : ' ');
            }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: field_check 64|128 < values\n");
        return 2;
    }
    return atoi(argv[1]) == 64 ? run<F64>() : run<F128>();
}
