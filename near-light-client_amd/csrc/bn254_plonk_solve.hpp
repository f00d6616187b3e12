// gnark's witness solver for a PLONK SparseR1CS over BN254: the schedule - one host pass over the
// constraints in index order that yields every item's form, level and assigned variable - and the per-item arithmetic on
// bnf::Fp<RP>, in one header that plain g++ builds (tests/native/bn254_plonk_solve_check.cpp) and that the kernels of
// bn254_plonk_solve.hip compile as it stands.  The rules are those of tools/gnark_plonk_solve_model.py, the place of record:
// RECALLED from gnark v0.9 (constraint/bn254/solver.go), UNPINNED; this header shares no code with the model.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "bn254_fp.hpp"

namespace nlx {
namespace plsolve {

typedef bnf::Fp<bnf::RP> Fr;

enum Form : uint32_t { CHECK = 0, SOLVE_L = 1, SOLVE_R = 2, SOLVE_O = 3, INV_ZERO = 4, N_BITS = 5, QUO_REM64 = 6, COMMIT = 7, SKIPPED = 8, N_FORMS = 8 };
enum Fail : uint32_t { OK = 0, DIV_ZERO = 1, UNSATISFIED = 2 };
enum State : uint8_t { UNASSIGNED = 0, ASSIGNED = 1, POISONED = 2 };
constexpr uint32_t NONE = 0xFFFFFFFFu;
// which coefficients of a constraint are nonzero, one bit each: the only thing the schedule needs of them
enum { NZ_L = 1, NZ_R = 2, NZ_M = 4, NZ_O = 8, NZ_K = 16 };
enum { CNT_L = 1, CNT_R = 2, CNT_O = 4 };

// rule 2: the cells whose coefficient can determine them
BNF_HD uint32_t counting(uint32_t nz) {
    return ((nz & (NZ_L | NZ_M)) ? CNT_L : 0) | ((nz & (NZ_R | NZ_M)) ? CNT_R : 0) | ((nz & NZ_O) ? CNT_O : 0);
}
BNF_HD uint32_t nonzero_bits(const Fr q[5]) {
    uint32_t nz = 0;
    for (int s = 0; s < 5; s++) nz |= bnf::is_zero(q[s]) ? 0u : 1u << s;
    return nz;
}

// ---- the arithmetic ----
BNF_HD Fr fr_inv(const Fr& a) {   // a^(r - 2): about 380 dependent products; 0 for 0
    Fr r = bnf::one<bnf::RP>();
#pragma unroll 1
    for (int bit = 253; bit >= 0; bit--) {
        r = bnf::sqr(r);
        const uint32_t word = bnf::RP::mod(bit >> 5) - ((bit >> 5) == 0 ? 2u : 0u);   // r ends in ...1: no borrow
        if ((word >> (bit & 31)) & 1) r = bnf::mul(r, a);
    }
    return r;
}

// One constraint (rule 4).  q = ql qr qm qo qk; an operand whose cell does not count, and the cell being solved, come as 0.
// inverted: the divisor is a coefficient alone and its slot of q (qo; ql or qr with qm = 0) already holds its INVERSE - the
// solver inverts those once, at creation.  -> the failure kind; `out` = the solved value, `value` = the numerator or the
// constraint's value (Montgomery).
BNF_HD uint32_t solve_item(uint32_t form, bool inverted, const Fr q[5], const Fr& l, const Fr& r, const Fr& o, Fr& out, Fr& value) {
    using namespace bnf;
    const Fr lr = mul(l, r);
    if (form == CHECK) {
        value = add(add(add(mul(q[0], l), mul(q[1], r)), add(mul(q[2], lr), mul(q[3], o))), q[4]);
        out = zero<RP>();
        return is_zero(value) ? OK : UNSATISFIED;
    }
    Fr div;
    if (form == SOLVE_O) {
        value = add(add(mul(q[0], l), mul(q[1], r)), add(mul(q[2], lr), q[4]));
        div = q[3];
    } else if (form == SOLVE_L) {
        value = add(add(mul(q[1], r), mul(q[3], o)), q[4]);
        div = inverted ? q[0] : add(q[0], mul(q[2], r));
    } else {
        value = add(add(mul(q[0], l), mul(q[3], o)), q[4]);
        div = inverted ? q[1] : add(q[1], mul(q[2], l));
    }
    out = zero<RP>();
    if (!inverted) {
        if (is_zero(div)) return DIV_ZERO;   // whatever the numerator (rule 8)
        div = fr_inv(div);
    }
    out = neg(mul(value, div));
    return OK;
}

// rule 5, the three arithmetic hints
BNF_HD Fr hint_inv_zero(const Fr& x) { return fr_inv(x); }   // 0^(r-2) = 0
// output i of N_BITS from the CANONICAL integer (bnf::from_mont(x)), i < 256
BNF_HD Fr hint_bit(const Fr& canonical, uint32_t i) {
    uint32_t word = 0;   // selects, not an indexed array: the limbs stay in registers
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) word = (i >> 5) == k ? canonical.v[k] : word;
    return ((word >> (i & 31)) & 1) ? bnf::one<bnf::RP>() : bnf::zero<bnf::RP>();
}
// canonical(x) = q m + rem, 0 <= rem < m, 1 <= m < 2^64: binary long division, the same text on both sides (the outer loop
// is unrolled so that every limb index is a constant)
BNF_HD void hint_quo_rem64(const Fr& x, uint64_t m, Fr& q, Fr& rem) {
    const Fr c = bnf::from_mont(x);
    Fr quo;
    uint64_t r = 0;
#pragma unroll
    for (int w = 7; w >= 0; w--) {
        const uint32_t cw = c.v[w];
        uint32_t qw = 0;
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            const uint64_t top = r >> 63;
            r = (r << 1) | ((cw >> bit) & 1);
            if (top || r >= m) {
                r -= m;
                qw |= 1u << bit;
            }
        }
        quo.v[w] = qw;
    }
    Fr rr = bnf::zero<bnf::RP>();
    rr.v[0] = (uint32_t)r, rr.v[1] = (uint32_t)(r >> 32);
    q = bnf::to_mont(quo);      // the quotient of an integer below r is below r
    rem = bnf::to_mont(rr);
}

// The poison rule.  An item one of whose counting operands (the cell being solved apart) is poisoned fails nothing and
// poisons what it would assign; a failing solve poisons its variable too.
BNF_HD bool poisoned_operand(uint32_t form, uint32_t counts, uint8_t sl, uint8_t sr, uint8_t so) {
    if (form == SOLVE_L) counts &= ~(uint32_t)CNT_L;
    if (form == SOLVE_R) counts &= ~(uint32_t)CNT_R;
    if (form == SOLVE_O) counts &= ~(uint32_t)CNT_O;
    return ((counts & CNT_L) && sl == POISONED) || ((counts & CNT_R) && sr == POISONED) || ((counts & CNT_O) && so == POISONED);
}
BNF_HD uint8_t state_after(bool operand_poisoned, uint32_t fail) { return operand_poisoned || fail != OK ? POISONED : ASSIGNED; }

// ---- the schedule (host) ----
struct Hint {
    uint32_t id = 0;                 // what a refusal calls it: the caller's index; n_listed + j for commitment j's
    uint32_t kind = 0, before = 0;   // INV_ZERO, N_BITS, QUO_REM64 as listed by the caller; COMMIT as the setup implies it (param = j)
    uint64_t param = 0;
    std::vector<uint32_t> in, out;
};
struct Item {
    uint32_t form, level, index;     // index: the constraint, or the hint in the list the schedule was made from
    uint32_t assigns;                // the variable a solve assigns, else NONE
    uint32_t x[3];                   // a constraint's cells; a hint's input variable, first output slot and output count
    bool const_div;
};
struct Schedule {
    std::vector<Item> items;                         // by level, then form, then index
    std::vector<uint32_t> level, form, assigns;      // per constraint (level 0, SKIPPED, NONE where skipped)
    std::vector<uint32_t> hint_level;                // per hint
    std::vector<uint32_t> hint_out;                  // the hints' outputs, concatenated
    std::vector<uint64_t> level_off;                 // items of level v: [level_off[v - 1], level_off[v]), v = 1 .. levels
    uint64_t unassigned = 0;
    uint32_t levels = 0;
};

// One pass in index order; assigners always come earlier, so the levels fall out of the same pass.  cells: [3][nc] variable ids
// (already checked below n_variables), nz: the NZ_* bits per constraint, skipped: nonzero where rule 3 applies.  The hints must
// come with `before` non-descending (a COMMIT after the listed hints of its `before`).  false: refused, `err` names the
// constraint or hint (rule 6).
inline bool make_schedule(uint64_t n_variables, uint64_t n_given, uint64_t nc, const uint32_t* const cells[3], const uint8_t* nz, const uint8_t* skipped,
                          const std::vector<Hint>& hints, Schedule& s, std::string& err) {
    char buf[200];
    constexpr int32_t NOT = -1;
    std::vector<int32_t> level_of((size_t)n_variables, NOT);
    for (uint64_t v = 0; v < n_given && v < n_variables; v++) level_of[(size_t)v] = 0;
    s.level.assign((size_t)nc, 0), s.form.assign((size_t)nc, SKIPPED), s.assigns.assign((size_t)nc, NONE);
    s.hint_level.assign(hints.size(), 0);
    s.items.clear(), s.hint_out.clear();
    uint32_t last = 0;
    for (size_t h = 0; h < hints.size(); h++) {
        const Hint& t = hints[h];
        const char* bad = nullptr;
        if (t.before < last || t.before > nc) bad = "`before` descends or exceeds the constraints";
        else if (t.kind < INV_ZERO || t.kind > COMMIT) bad = "unknown kind";
        else if (t.kind != COMMIT && t.in.size() != 1) bad = "takes one input";
        else if (t.kind == INV_ZERO && t.out.size() != 1) bad = "INV_ZERO gives one output";
        else if (t.kind == N_BITS && (t.out.empty() || t.out.size() > 256)) bad = "N_BITS gives 1 .. 256 outputs";
        else if (t.kind == QUO_REM64 && (t.out.size() != 2 || t.param == 0)) bad = "QUO_REM64 gives two outputs and takes 1 <= m < 2^64";
        for (uint32_t v : t.in) if (!bad && v >= n_variables) bad = "an input variable out of range";
        for (uint32_t v : t.out) if (!bad && v >= n_variables) bad = "an output variable out of range";
        if (bad) {
            snprintf(buf, sizeof buf, "hint %u (before = %u): %s", t.id, t.before, bad);
            err = buf;
            return false;
        }
        last = t.before;
    }
    size_t next_hint = 0;
    auto do_hints = [&](uint64_t before) -> bool {
        for (; next_hint < hints.size() && hints[next_hint].before == before; next_hint++) {
            const size_t h = next_hint;
            const Hint& t = hints[h];
            int32_t lv = 0;
            for (uint32_t v : t.in) {
                if (level_of[v] == NOT) {
                    snprintf(buf, sizeof buf, "hint %u: input variable %u is not assigned in front of constraint %llu", t.id, v, (unsigned long long)before);
                    err = buf;
                    return false;
                }
                lv = std::max(lv, level_of[v]);
            }
            lv++;
            for (uint32_t v : t.out) {
                if (level_of[v] != NOT) {
                    snprintf(buf, sizeof buf, "hint %u: output variable %u is given or assigned twice", t.id, v);
                    err = buf;
                    return false;
                }
                level_of[v] = lv;
            }
            s.hint_level[h] = (uint32_t)lv;
            Item it{t.kind, (uint32_t)lv, (uint32_t)h, NONE, {t.in.empty() ? 0u : t.in[0], (uint32_t)s.hint_out.size(), (uint32_t)t.out.size()}, false};
            if (t.kind == COMMIT) it.x[0] = (uint32_t)t.param;
            s.hint_out.insert(s.hint_out.end(), t.out.begin(), t.out.end());
            s.items.push_back(it);
        }
        return true;
    };
    for (uint64_t c = 0; c < nc; c++) {
        if (!do_hints(c)) return false;
        if (skipped && skipped[c]) continue;
        const uint32_t counts = counting(nz[c]);
        const uint32_t x[3] = {cells[0][c], cells[1][c], cells[2][c]};
        int32_t lv = 0;
        uint32_t unknown = NONE, where = 0, n_unknown = 0;
        for (uint32_t col = 0; col < 3; col++) {
            if (!(counts >> col & 1)) continue;
            if (level_of[x[col]] != NOT) {
                lv = std::max(lv, level_of[x[col]]);
                continue;
            }
            if (n_unknown && x[col] != unknown) {
                snprintf(buf, sizeof buf, "constraint %llu: two unassigned variables (%u, %u)", (unsigned long long)c, std::min(unknown, x[col]), std::max(unknown, x[col]));
                err = buf;
                return false;
            }
            if (!n_unknown) unknown = x[col], where = col;
            n_unknown++;
        }
        if (n_unknown > 1) {
            snprintf(buf, sizeof buf, "constraint %llu: variable %u is unassigned in two cells (quadratic)", (unsigned long long)c, unknown);
            err = buf;
            return false;
        }
        lv++;
        s.level[c] = (uint32_t)lv;
        Item it{CHECK, (uint32_t)lv, (uint32_t)c, NONE, {x[0], x[1], x[2]}, false};
        if (n_unknown) {
            it.form = SOLVE_L + where;
            it.assigns = unknown;
            it.const_div = it.form == SOLVE_O || !(nz[c] & NZ_M);
            level_of[unknown] = lv;
        }
        s.form[c] = it.form, s.assigns[c] = it.assigns;
        s.items.push_back(it);
    }
    if (!do_hints(nc)) return false;
    s.unassigned = 0;
    for (int32_t lv : level_of) s.unassigned += lv == NOT;
    std::stable_sort(s.items.begin(), s.items.end(), [](const Item& a, const Item& b) {
        if (a.level != b.level) return a.level < b.level;
        if (a.form != b.form) return a.form < b.form;
        return a.index < b.index;
    });
    s.levels = s.items.empty() ? 0 : s.items.back().level;
    s.level_off.assign((size_t)s.levels + 1, 0);
    for (const Item& it : s.items) s.level_off[it.level]++;
    for (uint32_t v = 1; v <= s.levels; v++) s.level_off[v] += s.level_off[v - 1];
    return true;
}

}  // namespace plsolve
}  // namespace nlx
