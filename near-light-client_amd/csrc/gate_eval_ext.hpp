// plonky2 gate constraints at a point of the quadratic extension: Gate::eval_unfiltered for the gate kinds include/nlx.h numbers
// 1 .. 18, and vanishing_poly::check_lookup_constraints, over gl::Ext.  The verifier's evaluator
// (plonk_verify.hip); eval_gate in prover_kernels.hip is the base-field one, tuned for the quotient kernel, and stays as it is.
//
// Host and device (same source): `wire(i)` / `cst(i)` return the opening of wire i / gate constant i at zeta, `emit(c)` takes
// the constraints in plonky2's order.  The gates whose wires ENCODE extension elements (ArithmeticExtension, MulExtension,
// Reducing, ReducingExtension, PoseidonMds, CosetInterpolation) multiply in the extension ALGEBRA: a pair of openings (c0, c1)
// stands for c0 + c1 X with X^2 = 7 over the extension itself, which is what the polynomial identity of the base-field
// constraints becomes once the wires are evaluated off the base field.
#pragma once
#include "gl.hpp"
#include "poseidon.hpp"
#include "prover.hpp"

namespace nlx {
namespace gext {

using gl::Ext;

GL_HD Ext base(uint64_t c) { return Ext{c, 0}; }
GL_HD Ext add_base(Ext x, uint64_t b) { return Ext{gl::add(x.a, b), x.b}; }
GL_HD Ext sub_base(Ext x, uint64_t b) { return Ext{gl::sub(x.a, b), x.b}; }
GL_HD Ext one_minus(Ext x) { return Ext{gl::sub(1, x.a), gl::neg(x.b)}; }
GL_HD Ext sqr(Ext x) { return gl::mul(x, x); }

// an element of the extension algebra
struct Alg {
    Ext c0, c1;
};
GL_HD Alg alg_mul(Alg x, Alg y) {
    const Ext t = gl::mul(x.c1, y.c1);
    return Alg{gl::add(gl::mul(x.c0, y.c0), gl::mul(t, gl::W)), gl::add(gl::mul(x.c0, y.c1), gl::mul(x.c1, y.c0))};
}

GL_HD Ext sbox7(Ext x) {
    const Ext x2 = sqr(x), x4 = sqr(x2), x3 = gl::mul(x, x2);
    return gl::mul(x3, x4);
}
// the Poseidon linear layer on twelve extension elements: the matrix is over the base field, so each coefficient goes alone
GL_HD void mds_layer(Ext (&s)[12]) {
    uint64_t a[12], b[12];
    for (int i = 0; i < 12; i++) { a[i] = s[i].a; b[i] = s[i].b; }
    poseidon::mds_layer(a);
    poseidon::mds_layer(b);
    for (int i = 0; i < 12; i++) s[i] = Ext{gl::canon(a[i]), gl::canon(b[i])};
}
// prod_{x < 4} (l - x): the 2-bit limb range check of the u32 gates
GL_HD Ext limb4(Ext l) {
    return gl::mul(gl::mul(l, sub_base(l, 1)), gl::mul(sub_base(l, 2), sub_base(l, 3)));
}
// prod_{x < count} (l - x)
GL_HD Ext range_product(Ext l, uint32_t count) {
    Ext p = base(1);
    for (uint32_t x = 0; x < count; x++) p = gl::mul(p, sub_base(l, x));
    return p;
}

// Gate::num_constraints
GL_HD uint32_t gate_num_constraints(const GateDev& g) {
    const uint32_t p0 = g.param0, p1 = g.param1;
    switch (g.kind) {
        case NLX_GATE_CONSTANT: case NLX_GATE_ARITHMETIC: return p0;
        case NLX_GATE_PUBLIC_INPUT: return 4;
        case NLX_GATE_BASE_SUM: return 1 + p1;
        case NLX_GATE_POSEIDON: return 123;
        case NLX_GATE_ARITHMETIC_EXT: case NLX_GATE_MUL_EXT: case NLX_GATE_REDUCING: case NLX_GATE_REDUCING_EXT: return 2 * p0;
        case NLX_GATE_POSEIDON_MDS: return 24;
        case NLX_GATE_EXPONENTIATION: return p0 + 1;
        case NLX_GATE_RANDOM_ACCESS: return (p1 & 0xFFFF) * (p0 + 2) + (p1 >> 16);
        case NLX_GATE_COSET_INTERPOLATION: return 2 * (2 + 2 * (((1u << p0) - 2) / (p1 - 1)));
        case NLX_GATE_U32_ADD_MANY: return p1 * (3 + 18);
        case NLX_GATE_U32_ARITHMETIC: return p0 * (4 + 32);
        case NLX_GATE_U32_SUBTRACTION: return p0 * (3 + 16);
        case NLX_GATE_U32_RANGE_CHECK: return p0 * 17;
        case NLX_GATE_COMPARISON: return 6 + 5 * p1 + (p0 + p1 - 1) / p1;
        default: return 0;
    }
}

// PoseidonGate.  Wires: input 0 .. 11, output 12 .. 23, swap 24, delta 25 .. 28, the S-box inputs of full rounds 1 .. 3 from 29,
// of the 22 partial rounds from 65, of the last four full rounds from 87.  The partial rounds run in their plain form (add the
// round's constants, element 0 through the S-box, the whole matrix): element 0 enters its S-box with the same value as in
// plonky2's fast form, so the constraints are the same polynomials.
template <class WireFn, class EmitFn>
GL_HD void poseidon_gate(WireFn& wire, EmitFn& emit) {
    const uint64_t* rc = poseidon::rc_table();
    const Ext swap = wire(24);
    emit(gl::mul(swap, sub_base(swap, 1)));
    Ext st[12];
    for (uint32_t i = 0; i < 4; i++) {
        const Ext lhs = wire(i), rhs = wire(i + 4), delta = wire(25 + i);
        emit(gl::sub(gl::mul(swap, gl::sub(rhs, lhs)), delta));
        st[i] = gl::add(lhs, delta);
        st[i + 4] = gl::sub(rhs, delta);
    }
    for (uint32_t i = 8; i < 12; i++) st[i] = wire(i);
    uint32_t round = 0;
    for (uint32_t r = 0; r < 4; r++, round++) {
        for (uint32_t i = 0; i < 12; i++) st[i] = add_base(st[i], rc[round * 12 + i]);
        if (r != 0)
            for (uint32_t i = 0; i < 12; i++) {
                const Ext in = wire(29 + 12 * (r - 1) + i);
                emit(gl::sub(st[i], in));
                st[i] = in;
            }
        for (uint32_t i = 0; i < 12; i++) st[i] = sbox7(st[i]);
        mds_layer(st);
    }
    for (uint32_t r = 0; r < 22; r++, round++) {
        for (uint32_t i = 0; i < 12; i++) st[i] = add_base(st[i], rc[round * 12 + i]);
        const Ext in = wire(65 + r);
        emit(gl::sub(st[0], in));
        st[0] = sbox7(in);
        mds_layer(st);
    }
    for (uint32_t r = 0; r < 4; r++, round++) {
        for (uint32_t i = 0; i < 12; i++) {
            const Ext in = wire(87 + 12 * r + i);
            emit(gl::sub(add_base(st[i], rc[round * 12 + i]), in));
            st[i] = sbox7(in);
        }
        mds_layer(st);
    }
    for (uint32_t i = 0; i < 12; i++) emit(gl::sub(st[i], wire(12 + i)));
}

// The constraints of gate `g` in plonky2's order.  pih: the public-inputs hash (base field).
template <class WireFn, class ConstFn, class EmitFn>
GL_HD void eval_gate_ext(const GateDev& g, WireFn& wire, ConstFn& cst, const uint64_t pih[4], EmitFn& emit) {
    const uint32_t p0 = g.param0, p1 = g.param1;
    switch (g.kind) {
        case NLX_GATE_CONSTANT:
            for (uint32_t i = 0; i < p0; i++) emit(gl::sub(cst(i), wire(i)));
            break;
        case NLX_GATE_PUBLIC_INPUT:
            for (uint32_t i = 0; i < 4; i++) emit(sub_base(wire(i), pih[i]));
            break;
        case NLX_GATE_ARITHMETIC: {   // output = c0 m0 m1 + c1 addend
            const Ext c0 = cst(0), c1 = cst(1);
            for (uint32_t i = 0; i < p0; i++) {
                const Ext prod = gl::mul(gl::mul(wire(4 * i), wire(4 * i + 1)), c0);
                emit(gl::sub(wire(4 * i + 3), gl::add(prod, gl::mul(wire(4 * i + 2), c1))));
            }
            break;
        }
        case NLX_GATE_BASE_SUM: {     // base p0, p1 limbs, little-endian on wires 1 ..
            Ext acc = base(0);
            for (uint32_t i = p1; i-- > 0;) acc = gl::add(gl::mul(acc, (uint64_t)p0), wire(1 + i));
            emit(gl::sub(acc, wire(0)));
            for (uint32_t i = 0; i < p1; i++) emit(range_product(wire(1 + i), p0));
            break;
        }
        case NLX_GATE_POSEIDON: poseidon_gate(wire, emit); break;
        case NLX_GATE_ARITHMETIC_EXT: {   // output = c0 m0 m1 + c1 addend, each an algebra element on two wires
            const Ext c0 = cst(0), c1 = cst(1);
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t w = 8 * i;
                const Alg p = alg_mul(Alg{wire(w), wire(w + 1)}, Alg{wire(w + 2), wire(w + 3)});
                emit(gl::sub(wire(w + 6), gl::add(gl::mul(p.c0, c0), gl::mul(wire(w + 4), c1))));
                emit(gl::sub(wire(w + 7), gl::add(gl::mul(p.c1, c0), gl::mul(wire(w + 5), c1))));
            }
            break;
        }
        case NLX_GATE_MUL_EXT: {
            const Ext c0 = cst(0);
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t w = 6 * i;
                const Alg p = alg_mul(Alg{wire(w), wire(w + 1)}, Alg{wire(w + 2), wire(w + 3)});
                emit(gl::sub(wire(w + 4), gl::mul(p.c0, c0)));
                emit(gl::sub(wire(w + 5), gl::mul(p.c1, c0)));
            }
            break;
        }
        case NLX_GATE_REDUCING:
        case NLX_GATE_REDUCING_EXT: {   // acc_i = acc_(i-1) alpha + coeff_i; output 0 .. 1, alpha 2 .. 3, old acc 4 .. 5, coefficients from 6
            const bool ext = g.kind == NLX_GATE_REDUCING_EXT;
            const uint32_t coeffs0 = 6, accs0 = coeffs0 + (ext ? 2 * p0 : p0);
            const Alg alpha{wire(2), wire(3)};
            Alg acc{wire(4), wire(5)};
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t at = i + 1 == p0 ? 0 : accs0 + 2 * i;   // the last accumulator is the output
                const Alg next{wire(at), wire(at + 1)};
                const Alg p = alg_mul(acc, alpha);
                if (ext) {
                    emit(gl::sub(gl::add(p.c0, wire(coeffs0 + 2 * i)), next.c0));
                    emit(gl::sub(gl::add(p.c1, wire(coeffs0 + 2 * i + 1)), next.c1));
                } else {
                    emit(gl::sub(gl::add(p.c0, wire(coeffs0 + i)), next.c0));
                    emit(gl::sub(p.c1, next.c1));
                }
                acc = next;
            }
            break;
        }
        case NLX_GATE_POSEIDON_MDS: {   // twelve algebra elements in (wires 2 i, 2 i + 1), the matrix times them out (from wire 24)
            constexpr uint32_t C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
            for (uint32_t r = 0; r < 12; r++) {
                Ext c0 = base(0), c1 = base(0);
                for (uint32_t i = 0; i < 12; i++) {
                    const uint32_t e = (i + r) % 12;
                    const uint64_t k = C[i] + (r == 0 && i == 0 ? 8u : 0u);
                    c0 = gl::add(c0, gl::mul(wire(2 * e), k));
                    c1 = gl::add(c1, gl::mul(wire(2 * e + 1), k));
                }
                emit(gl::sub(wire(24 + 2 * r), c0));
                emit(gl::sub(wire(24 + 2 * r + 1), c1));
            }
            break;
        }
        case NLX_GATE_EXPONENTIATION: {   // base 0, bits 1 .. p0 (little-endian), output 1 + p0, intermediates from 2 + p0
            const Ext b = wire(0);
            for (uint32_t i = 0; i < p0; i++) {
                const Ext prev = i ? sqr(wire(2 + p0 + i - 1)) : base(1);
                const Ext bit = wire(1 + (p0 - 1 - i));
                const Ext sel = gl::add(gl::mul(bit, b), one_minus(bit));
                emit(gl::sub(gl::mul(prev, sel), wire(2 + p0 + i)));
            }
            emit(gl::sub(wire(1 + p0), wire(2 + p0 + p0 - 1)));
            break;
        }
        case NLX_GATE_RANDOM_ACCESS: {
            const uint32_t bits = p0, copies = p1 & 0xFFFF, extra = p1 >> 16, vec = 1u << bits;
            const uint32_t routed = (2 + vec) * copies + extra;
            for (uint32_t cpy = 0; cpy < copies; cpy++) {
                const uint32_t b0 = (2 + vec) * cpy, bw = routed + cpy * bits;
                Ext rec = base(0);
                for (uint32_t i = 0; i < bits; i++) {
                    const Ext bit = wire(bw + i);
                    emit(gl::mul(bit, sub_base(bit, 1)));
                }
                for (uint32_t i = bits; i-- > 0;) rec = gl::add(gl::add(rec, rec), wire(bw + i));
                emit(gl::sub(rec, wire(b0)));
                // the list folded pair by pair with bit 0, then bit 1, ... is its multilinear extension at the bits: entry k
                // weighs prod_i (bit_i if k has bit i, else 1 - bit_i) - the same polynomial, without the list in registers
                Ext picked = base(0);
                for (uint32_t k = 0; k < vec; k++) {
                    Ext wgt = wire(b0 + 2 + k);
                    for (uint32_t i = 0; i < bits; i++) {
                        const Ext bit = wire(bw + i);
                        wgt = gl::mul(wgt, (k >> i) & 1 ? bit : one_minus(bit));
                    }
                    picked = gl::add(picked, wgt);
                }
                emit(gl::sub(picked, wire(b0 + 1)));
            }
            for (uint32_t i = 0; i < extra; i++) emit(gl::sub(cst(i), wire((2 + vec) * copies + i)));
            break;
        }
        case NLX_GATE_COSET_INTERPOLATION: {
            // shift 0, 2^bits algebra values from 1, evaluation point, evaluation value, the chunks' intermediate (eval, prod)
            // pairs, the shifted point; barycentric weights of the subgroup of order N: w_j = x_j / N
            const uint32_t np = 1u << p0, deg = p1;
            const uint32_t w_point = 1 + 2 * np, w_value = w_point + 2, w_inter = w_value + 2, ni = (np - 2) / (deg - 1);
            const uint32_t w_shifted = w_inter + 4 * ni;
            const Ext shift = wire(0);
            const Alg pt{wire(w_shifted), wire(w_shifted + 1)};
            emit(gl::sub(wire(w_point), gl::mul(pt.c0, shift)));
            emit(gl::sub(wire(w_point + 1), gl::mul(pt.c1, shift)));
            const uint64_t gen = gl::root_of_unity(p0), inv_np = gl::inv((uint64_t)np);
            Alg ev{base(0), base(0)}, prod{base(1), base(0)};
            uint64_t x = 1;
            uint32_t j = 0;
            for (uint32_t c = 0; c <= ni; c++) {
                uint32_t end = c == 0 ? deg : 1 + (deg - 1) * c + deg - 1;
                if (end > np) end = np;
                for (; j < end; j++) {
                    const Alg term{sub_base(pt.c0, x), pt.c1};
                    const uint64_t wj = gl::mul(x, inv_np);
                    const Alg a = alg_mul(ev, term), b = alg_mul(Alg{wire(1 + 2 * j), wire(2 + 2 * j)}, prod);
                    ev = Alg{gl::add(a.c0, gl::mul(b.c0, wj)), gl::add(a.c1, gl::mul(b.c1, wj))};
                    prod = alg_mul(prod, term);
                    x = gl::mul(x, gen);
                }
                if (c < ni) {
                    const Alg ie{wire(w_inter + 2 * c), wire(w_inter + 2 * c + 1)};
                    const Alg ip{wire(w_inter + 2 * (ni + c)), wire(w_inter + 2 * (ni + c) + 1)};
                    emit(gl::sub(ie.c0, ev.c0));
                    emit(gl::sub(ie.c1, ev.c1));
                    emit(gl::sub(ip.c0, prod.c0));
                    emit(gl::sub(ip.c1, prod.c1));
                    ev = ie;
                    prod = ip;
                }
            }
            emit(gl::sub(wire(w_value), ev.c0));
            emit(gl::sub(wire(w_value + 1), ev.c1));
            break;
        }
        case NLX_GATE_U32_ADD_MANY: {   // p0 addends + carry = out_carry 2^32 + out_result; 16 + 2 two-bit limbs
            const uint32_t na = p0, nops = p1;
            for (uint32_t i = 0; i < nops; i++) {
                const uint32_t w = (na + 3) * i, lb = (na + 3) * nops + 18 * i;
                Ext computed = wire(w + na);
                for (uint32_t k = 0; k < na; k++) computed = gl::add(computed, wire(w + k));
                const Ext res = wire(w + na + 1), cy = wire(w + na + 2);
                emit(gl::sub(gl::add(gl::mul(cy, (uint64_t)1 << 32), res), computed));
                Ext cr = base(0), cc = base(0);
                for (uint32_t k = 18; k-- > 0;) {
                    const Ext l = wire(lb + k);
                    emit(limb4(l));
                    if (k < 16) cr = gl::add(gl::mul(cr, (uint64_t)4), l);
                    else cc = gl::add(gl::mul(cc, (uint64_t)4), l);
                }
                emit(gl::sub(cr, res));
                emit(gl::sub(cc, cy));
            }
            break;
        }
        case NLX_GATE_U32_ARITHMETIC: {   // m0 m1 + addend = high 2^32 + low, high 2^32 + low canonical
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t w = 6 * i, lb = 6 * p0 + 32 * i;
                const Ext computed = gl::add(gl::mul(wire(w), wire(w + 1)), wire(w + 2));
                const Ext lo = wire(w + 3), hi = wire(w + 4), inv = wire(w + 5);
                const Ext diff = Ext{gl::sub(0xFFFFFFFFULL, hi.a), gl::neg(hi.b)};
                emit(gl::mul(sub_base(gl::mul(inv, diff), 1), lo));
                emit(gl::sub(gl::add(gl::mul(hi, (uint64_t)1 << 32), lo), computed));
                Ext cl = base(0), ch = base(0);
                for (uint32_t k = 32; k-- > 0;) {
                    const Ext l = wire(lb + k);
                    emit(limb4(l));
                    if (k < 16) cl = gl::add(gl::mul(cl, (uint64_t)4), l);
                    else ch = gl::add(gl::mul(ch, (uint64_t)4), l);
                }
                emit(gl::sub(cl, lo));
                emit(gl::sub(ch, hi));
            }
            break;
        }
        case NLX_GATE_U32_SUBTRACTION: {   // x - y - borrow_in + 2^32 borrow_out = result
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t w = 5 * i, lb = 5 * p0 + 16 * i;
                const Ext initial = gl::sub(gl::sub(wire(w), wire(w + 1)), wire(w + 2));
                const Ext res = wire(w + 3), bo = wire(w + 4);
                emit(gl::sub(res, gl::add(initial, gl::mul(bo, (uint64_t)1 << 32))));
                Ext c = base(0);
                for (uint32_t k = 16; k-- > 0;) {
                    const Ext l = wire(lb + k);
                    emit(limb4(l));
                    c = gl::add(gl::mul(c, (uint64_t)4), l);
                }
                emit(gl::sub(c, res));
                emit(gl::mul(bo, one_minus(bo)));
            }
            break;
        }
        case NLX_GATE_U32_RANGE_CHECK: {
            for (uint32_t i = 0; i < p0; i++) {
                const uint32_t aux = p0 + 16 * i;
                Ext sum = base(0);
                for (uint32_t k = 16; k-- > 0;) sum = gl::add(gl::mul(sum, (uint64_t)4), wire(aux + k));
                emit(gl::sub(sum, wire(i)));
                for (uint32_t k = 0; k < 16; k++) emit(limb4(wire(aux + k)));
            }
            break;
        }
        case NLX_GATE_COMPARISON: {   // result = (first <= second), by the most significant chunk that differs
            const uint32_t nch = p1, cb = (p0 + nch - 1) / nch;
            const uint32_t fc = 4, sc = 4 + nch, eqd = 4 + 2 * nch, ceq = 4 + 3 * nch, iv = 4 + 4 * nch, msb = 4 + 5 * nch;
            Ext fcomb = base(0), scomb = base(0);
            for (uint32_t i = nch; i-- > 0;) {
                fcomb = gl::add(gl::mul(fcomb, (uint64_t)1 << cb), wire(fc + i));
                scomb = gl::add(gl::mul(scomb, (uint64_t)1 << cb), wire(sc + i));
            }
            emit(gl::sub(fcomb, wire(0)));
            emit(gl::sub(scomb, wire(1)));
            Ext msd = base(0);
            for (uint32_t i = 0; i < nch; i++) {
                const Ext f = wire(fc + i), s = wire(sc + i), eq = wire(ceq + i), v = wire(iv + i);
                emit(range_product(f, 1u << cb));
                emit(range_product(s, 1u << cb));
                const Ext diff = gl::sub(s, f);
                emit(gl::sub(gl::mul(diff, wire(eqd + i)), one_minus(eq)));
                emit(gl::mul(eq, diff));
                emit(gl::sub(v, gl::mul(eq, msd)));
                msd = gl::add(v, gl::mul(one_minus(eq), diff));
            }
            emit(gl::sub(wire(3), msd));
            Ext bc = base(0);
            for (uint32_t b = 0; b <= cb; b++) {
                const Ext bit = wire(msb + b);
                emit(gl::mul(bit, one_minus(bit)));
            }
            for (uint32_t b = cb + 1; b-- > 0;) bc = gl::add(gl::add(bc, bc), wire(msb + b));
            emit(gl::sub(add_base(wire(3), (uint64_t)1 << cb), bc));
            emit(gl::sub(wire(2), wire(msb + cb)));
            break;
        }
        default: break;   // NoopGate, LookupGate, LookupTableGate: no gate constraints
    }
}

// vanishing_poly::check_lookup_constraints for one challenge round: 4 + tables + 2 S constraints.  sel(i): the lookup selectors
// (TransSre, TransLdc, InitSre, LastLdc, then one per table); lz(i) / lz_next(i): the round's 1 + S lookup polynomials (RE, then
// the partial sums) at zeta / g zeta; deltas: (A, B, alpha, delta); lut_poly[t]: get_lut_poly of table t under them.
template <class WireFn, class SelFn, class LzFn, class LzNextFn, class EmitFn>
GL_HD void eval_lookup_ext(const LookupShape& s, WireFn& wire, SelFn& sel, LzFn& lz, LzNextFn& lz_next, const uint64_t deltas[4],
                           const uint64_t* lut_poly, EmitFn& emit) {
    const uint64_t dA = deltas[0], dB = deltas[1], alpha = deltas[2], delta = deltas[3];
    const uint32_t S = s.n_sldc;
    const Ext trans_sre = sel(0), trans_ldc = sel(1), init_sre = sel(2), last_ldc = sel(3), re = lz(0);
    emit(gl::mul(last_ldc, lz(S)));       // the running difference ends at 0
    emit(gl::mul(init_sre, lz(1)));       // the sum starts at 0 ...
    emit(gl::mul(init_sre, re));          // ... and so does RE
    for (uint32_t t = 0; t < s.num_luts; t++) emit(gl::mul(sel(4 + t), sub_base(re, lut_poly[t])));
    {
        Ext cur = lz_next(0);             // RE's row transition: Horner in delta over the row's table slots
        for (uint32_t i = 0; i < s.n_lut_slots; i++)
            cur = gl::add(gl::mul(cur, delta), gl::add(wire(3 * i), gl::mul(wire(3 * i + 1), dB)));
        emit(gl::mul(trans_sre, gl::sub(re, cur)));
    }
    // alpha - (input + A output) of table slot i / lookup slot i
    auto looked = [&](uint32_t i) { return Ext{gl::sub(alpha, gl::add(wire(3 * i).a, gl::mul(wire(3 * i + 1).a, dA))),
                                               gl::neg(gl::add(wire(3 * i).b, gl::mul(wire(3 * i + 1).b, dA)))}; };
    auto looking = [&](uint32_t i) { return Ext{gl::sub(alpha, gl::add(wire(2 * i).a, gl::mul(wire(2 * i + 1).a, dA))),
                                                gl::neg(gl::add(wire(2 * i).b, gl::mul(wire(2 * i + 1).b, dA)))}; };
    for (uint32_t p = 0; p < S; p++) {
        const uint32_t t0 = p * s.lut_degree, t1 = (p + 1) * s.lut_degree < s.n_lut_slots ? (p + 1) * s.lut_degree : s.n_lut_slots;
        const uint32_t u0 = p * s.lu_degree, u1 = (p + 1) * s.lu_degree < s.n_lu_slots ? (p + 1) * s.lu_degree : s.n_lu_slots;
        Ext lut_prod = base(1), lu_prod = base(1), lut_sum = base(0), lu_sum = base(0);
        for (uint32_t i = t0; i < t1; i++) lut_prod = gl::mul(lut_prod, looked(i));
        for (uint32_t i = u0; i < u1; i++) lu_prod = gl::mul(lu_prod, looking(i));
        for (uint32_t i = t0; i < t1; i++) {   // sum_i multiplicity_i prod_(j != i) (alpha - looked_j)
            Ext pr = wire(3 * i + 2);
            for (uint32_t j = t0; j < t1; j++)
                if (j != i) pr = gl::mul(pr, looked(j));
            lut_sum = gl::add(lut_sum, pr);
        }
        for (uint32_t i = u0; i < u1; i++) {   // sum_i prod_(j != i) (alpha - looking_j)
            Ext pr = base(1);
            for (uint32_t j = u0; j < u1; j++)
                if (j != i) pr = gl::mul(pr, looking(j));
            lu_sum = gl::add(lu_sum, pr);
        }
        // the partial sum before this one: in this row, or the last one of the next row (the rows run upside down)
        const Ext step = gl::sub(lz(1 + p), p == 0 ? lz_next(S) : lz(p));
        emit(gl::mul(trans_sre, gl::sub(gl::mul(lut_prod, step), lut_sum)));
        emit(gl::mul(trans_ldc, gl::add(gl::mul(lu_prod, step), lu_sum)));
    }
}

}  // namespace gext
}  // namespace nlx
