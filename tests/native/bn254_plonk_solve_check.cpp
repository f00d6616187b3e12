// Host check of csrc/bn254_plonk_solve.hpp with plain g++ (no HIP): the schedule and the per-item arithmetic the kernels of
// bn254_plonk_solve.hip compile, run as ONE sequential loop over the items in level order - the device's semantics (state bytes,
// the poison rule, the lowest failing constraint) on one core - against records computed by tools/gnark_plonk_solve_model.py
// (tests/test_bn254_plonk_solve_native_cpu.py writes them).  Field elements are 64 hex digits, Montgomery unless said otherwise.
//   circuit NV NGIVEN NC NH          starts a circuit; then NC lines  con XA XB XC SKIPPED QL QR QM QO QK
//                                    and NH lines  hint ID KIND BEFORE PARAM(16 hex) VALUE NIN in.. NOUT out..   in running order;
//                                    VALUE is what a COMMIT hint gives (the model's c_j), 0 otherwise
//   refuse WHICH INDEX               the schedule must refuse and name "constraint INDEX" (WHICH = 0) or "hint INDEX" (1)
//   sched  (LEVEL FORM ASSIGNS) x NC (LEVEL) x NH
//   run    NGIVEN inputs = KIND CONSTRAINT VALUE(canonical) FAILURES POISONED  NV values ("P" where poisoned)
// Prints "<records> cases, <bad> bad"; exit status 1 if any is bad.  With --time FILE: the seconds one sequential solve of the
// first circuit's first run takes (the median of five), for tools/plonk_solve_timing.py.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "bn254_plonk_solve.hpp"

using namespace nlx;
using namespace nlx::plsolve;

static Fr parse_fr(const std::string& s) {
    uint64_t w[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < s.size() && i < 64; i++) {
        const char ch = s[s.size() - 1 - i];
        const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        w[i / 16] |= d << (4 * (i % 16));
    }
    return bnf::load_words<bnf::RP>(w);
}

struct Circuit {
    uint64_t nv = 0, n_given = 0, nc = 0;
    std::vector<uint32_t> x[3];
    std::vector<uint8_t> skipped, nz;
    std::vector<Fr> q;           // [nc][5]
    std::vector<Hint> hints;
    std::vector<Fr> hint_value;
    Schedule sc;
    std::string err;
    bool ok = false;
    std::vector<Fr> item_q;      // [items][5], the constant divisors inverted
};

static void finish(Circuit& c) {
    const uint32_t* cells[3] = {c.x[0].data(), c.x[1].data(), c.x[2].data()};
    c.ok = make_schedule(c.nv, c.n_given, c.nc, cells, c.nz.data(), c.skipped.data(), c.hints, c.sc, c.err);
    if (!c.ok) return;
    c.item_q.assign(c.sc.items.size() * 5, bnf::zero<bnf::RP>());
    for (size_t i = 0; i < c.sc.items.size(); i++) {
        const Item& it = c.sc.items[i];
        if (it.form > SOLVE_O) continue;
        for (int s = 0; s < 5; s++) c.item_q[5 * i + s] = c.q[5 * (size_t)it.index + s];
        if (it.const_div) {
            Fr& d = c.item_q[5 * i + (it.form == SOLVE_O ? 3 : it.form == SOLVE_L ? 0 : 1)];
            d = fr_inv(d);
        }
    }
}

struct Outcome {
    uint32_t kind = 0, constraint = NONE;
    Fr value = bnf::zero<bnf::RP>();
    uint64_t failures = 0, poisoned = 0;
};

// the device's loop on one core
static Outcome solve(const Circuit& c, std::vector<Fr>& values, std::vector<uint8_t>& state) {
    Outcome out;
    auto put = [&](uint32_t v, uint8_t st, const Fr& x) {
        values[v] = st == ASSIGNED ? x : bnf::zero<bnf::RP>();
        state[v] = st;
        out.poisoned += st == POISONED;
    };
    for (size_t i = 0; i < c.sc.items.size(); i++) {
        const Item& it = c.sc.items[i];
        if (it.form <= SOLVE_O) {
            const Fr* q = &c.item_q[5 * i];
            uint32_t ops = counting(nonzero_bits(q));
            if (it.form != CHECK) ops &= ~(1u << (it.form - SOLVE_L));
            Fr op[3];
            uint8_t st[3];
            for (int k = 0; k < 3; k++) {
                const bool counts = ops >> k & 1;
                op[k] = counts ? values[it.x[k]] : bnf::zero<bnf::RP>();
                st[k] = counts ? state[it.x[k]] : (uint8_t)ASSIGNED;
            }
            const bool poisoned = poisoned_operand(it.form, ops, st[0], st[1], st[2]);
            Fr res = bnf::zero<bnf::RP>(), value = bnf::zero<bnf::RP>();
            const uint32_t fail = poisoned ? (uint32_t)OK : solve_item(it.form, it.const_div, q, op[0], op[1], op[2], res, value);
            if (it.form != CHECK) put(it.assigns, state_after(poisoned, fail), res);
            if (fail != OK) {
                out.failures++;
                if (it.index < out.constraint) out.constraint = it.index, out.kind = fail, out.value = bnf::from_mont(value);
            }
            continue;
        }
        const Hint& h = c.hints[it.index];
        bool poisoned = false;
        for (uint32_t v : h.in) poisoned |= state[v] == POISONED;
        const uint8_t st = poisoned ? (uint8_t)POISONED : (uint8_t)ASSIGNED;
        const uint32_t* outs = &c.sc.hint_out[it.x[1]];
        if (it.form == COMMIT) {
            put(outs[0], st, c.hint_value[it.index]);
        } else if (it.form == INV_ZERO) {
            put(outs[0], st, hint_inv_zero(values[it.x[0]]));
        } else if (it.form == N_BITS) {
            const Fr canonical = bnf::from_mont(values[it.x[0]]);
            for (uint32_t b = 0; b < it.x[2]; b++) put(outs[b], st, hint_bit(canonical, b));
        } else {
            Fr quo, rem;
            hint_quo_rem64(values[it.x[0]], h.param, quo, rem);
            put(outs[0], st, quo);
            put(outs[1], st, rem);
        }
    }
    return out;
}

int main(int argc, char** argv) {
    const bool timing = argc == 3 && !strcmp(argv[1], "--time");
    if (argc != 2 && !timing) {
        fprintf(stderr, "usage: %s [--time] cases.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[argc - 1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[argc - 1]);
        return 2;
    }
    Circuit c;
    size_t want_con = 0, want_hint = 0;
    bool finished = false;
    int records = 0, bad = 0;
    std::string line, tok;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> tok)) continue;
        if (tok == "circuit") {
            c = Circuit();
            uint64_t nh;
            ls >> c.nv >> c.n_given >> c.nc >> nh;
            want_con = (size_t)c.nc, want_hint = (size_t)nh;
            finished = false;
            continue;
        }
        if (tok == "con") {
            uint32_t a, b, o, sk;
            ls >> a >> b >> o >> sk;
            if (a >= c.nv || b >= c.nv || o >= c.nv || !want_con) {
                fprintf(stderr, "bad record: %s\n", line.c_str());
                return 2;
            }
            c.x[0].push_back(a), c.x[1].push_back(b), c.x[2].push_back(o), c.skipped.push_back((uint8_t)sk);
            Fr q[5];
            for (int s = 0; s < 5; s++) {
                ls >> tok;
                q[s] = parse_fr(tok);
                c.q.push_back(q[s]);
            }
            c.nz.push_back((uint8_t)nonzero_bits(q));
            want_con--;
            continue;
        }
        if (tok == "hint") {
            Hint h;
            std::string param, value;
            size_t n_in, n_out;
            ls >> h.id >> h.kind >> h.before >> param >> value >> n_in;
            h.param = strtoull(param.c_str(), nullptr, 16);
            h.in.resize(n_in);
            for (uint32_t& v : h.in) ls >> v;
            ls >> n_out;
            h.out.resize(n_out);
            for (uint32_t& v : h.out) ls >> v;
            if (!ls || !want_hint) {
                fprintf(stderr, "bad record: %s\n", line.c_str());
                return 2;
            }
            c.hints.push_back(h);
            c.hint_value.push_back(parse_fr(value));
            want_hint--;
            continue;
        }
        if (want_con || want_hint) {
            fprintf(stderr, "the circuit is incomplete at: %s\n", tok.c_str());
            return 2;
        }
        if (!finished) finish(c), finished = true;
        records++;
        bool good = true;
        if (tok == "refuse") {
            int which;
            unsigned index;
            ls >> which >> index;
            char want[64];
            snprintf(want, sizeof want, "%s %u", which ? "hint" : "constraint", index);
            const size_t at = c.err.find(want);
            good = !c.ok && at == 0 && (c.err[strlen(want)] == ':' || c.err[strlen(want)] == ' ');
            if (!good) printf("BAD refuse %s: ok = %d, message \"%s\"\n", want, (int)c.ok, c.err.c_str());
        } else if (tok == "sched") {
            good = c.ok;
            for (size_t i = 0; good && i < c.nc; i++) {
                uint32_t lv, form, assigns;
                ls >> lv >> form >> assigns;
                good = lv == c.sc.level[i] && form == c.sc.form[i] && assigns == c.sc.assigns[i];
                if (!good) printf("BAD sched constraint %zu: level %u form %u assigns %u, want %u %u %u\n", i, c.sc.level[i], c.sc.form[i], c.sc.assigns[i], lv, form, assigns);
            }
            for (size_t h = 0; good && h < c.hints.size(); h++) {
                uint32_t lv;
                ls >> lv;
                good = lv == c.sc.hint_level[h];
                if (!good) printf("BAD sched hint %zu: level %u, want %u\n", h, c.sc.hint_level[h], lv);
            }
            if (!c.ok) printf("BAD sched: refused, \"%s\"\n", c.err.c_str());
        } else if (tok == "run") {
            if (!c.ok) {
                printf("BAD run: the schedule was refused, \"%s\"\n", c.err.c_str());
                bad++;
                continue;
            }
            std::vector<Fr> inputs((size_t)c.n_given);
            for (Fr& x : inputs) {
                ls >> tok;
                x = parse_fr(tok);
            }
            auto once = [&](std::vector<Fr>& values, std::vector<uint8_t>& state) {
                values.assign((size_t)c.nv, bnf::zero<bnf::RP>());
                state.assign((size_t)c.nv, UNASSIGNED);
                for (size_t v = 0; v < c.n_given; v++) values[v] = inputs[v], state[v] = ASSIGNED;
                return solve(c, values, state);
            };
            std::vector<Fr> values;
            std::vector<uint8_t> state;
            if (timing) {
                double t[5];
                for (double& s : t) {
                    const auto t0 = std::chrono::steady_clock::now();
                    once(values, state);
                    s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                }
                std::sort(t, t + 5);
                printf("%.6f seconds per sequential solve of %zu items\n", t[2], c.sc.items.size());
                return 0;
            }
            const Outcome got = once(values, state);
            uint32_t kind, constraint;
            uint64_t failures, poisoned;
            std::string value;
            ls >> tok >> kind >> constraint >> value >> failures >> poisoned;
            good = tok == "=" && got.kind == kind && got.constraint == constraint && bnf::equal(got.value, parse_fr(value)) && got.failures == failures &&
                   got.poisoned == poisoned;
            if (!good) printf("BAD run: kind %u constraint %u failures %llu poisoned %llu, want %u %u %llu %llu\n", got.kind, got.constraint,
                              (unsigned long long)got.failures, (unsigned long long)got.poisoned, kind, constraint, (unsigned long long)failures, (unsigned long long)poisoned);
            for (size_t v = 0; good && v < c.nv; v++) {
                ls >> tok;
                good = tok == "P" ? state[v] == POISONED : state[v] != POISONED && bnf::equal(values[v], parse_fr(tok));
                if (!good) printf("BAD run: variable %zu (state %u)\n", v, state[v]);
            }
            if (!ls) good = false;
        } else {
            fprintf(stderr, "unknown record: %s\n", tok.c_str());
            return 2;
        }
        bad += !good;
    }
    printf("%d cases, %d bad\n", records, bad);
    return bad != 0;
}
