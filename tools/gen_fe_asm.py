#!/usr/bin/env python3
"""Generates narwhal_amd/csrc/fe_asm.h: the product parts of fe_mul / fe_sq / fe_sq2 as single
inline-asm blocks of v_mad_i64_i32.

Why asm: left to itself the compiler (a) pulls the carry-rounding bias out of each column's
multiply-accumulate chain and adds it afterwards with a separate 64-bit add, and (b) splits each
10-term chain into partial sums that it re-adds (another 64-bit add each) -- ~16 extra VOP3 ops
per multiply.  Here every column is exactly one chain of v_mad_i64_i32 whose first addend is the
column bias (an SGPR pair), and the chains of the 10 columns are issued round-robin so that
consecutive instructions are independent (dependency distance 10 for fe_mul, >= 5 for fe_sq).

Also generates narwhal_amd/csrc/feu_asm.h, the products of the non-negative field (fe_u25519.h):
the same columns as v_mad_u64_u32 chains, each seeded with the previous column's carry (emit_u).

Column layout (radix 2^25.5, see fe25519.h): column k collects f_i g_j with i + j = k (mod 10);
a wrapped product (i + j >= 10) carries 19, a product of two odd limbs carries 2.
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "narwhal_amd", "csrc", "fe_asm.h")


def mul_terms():
    cols = []
    for k in range(10):
        t = []
        for i in range(10):
            j = (k - i + 10) % 10
            wrap = i + j >= 10
            oo = (i & 1) and (j & 1)
            t.append(("f2_%d" % i if oo else "f_%d" % i, "g19_%d" % j if wrap else "g_%d" % j))
        cols.append(t)
    return cols


def sq_terms(double):
    """f^2 (or 2 f^2): off-diagonal terms carry 2 on the left factor; odd-odd 2 and wrap 19 on
    the right factor (as fe_sq_wide).  double: every left factor is doubled once more."""
    cols = [[] for _ in range(10)]
    for i in range(10):
        for j in range(i, 10):
            k = (i + j) % 10
            wrap = i + j >= 10
            oo = (i & 1) and (j & 1)
            lmul = (1 if i == j else 2) * (2 if double else 1)
            left = "f_%d" % i if lmul == 1 else "f%d_%d" % (lmul, i)
            if wrap:
                right = "f38_%d" % j if oo else "f19_%d" % j
            else:
                right = "f2_%d" % j if oo else "f_%d" % j
            cols[k].append((left, right))
    return cols


def emit(name, cols, doc):
    names = []
    for c in cols:
        for a, b in c:
            for x in (a, b):
                if x not in names:
                    names.append(x)
    idx = {n: 12 + i for i, n in enumerate(names)}   # %0..%9 outputs, %10 %11 biases
    depth = max(len(c) for c in cols)
    lines = []
    for r in range(depth):
        for k in range(10):
            if r >= len(cols[k]):
                continue
            a, b = cols[k][r]
            src2 = ("%%%d" % (10 + (k & 1))) if r == 0 else ("%%%d" % k)
            lines.append("v_mad_i64_i32 %%%d, vcc, %%%d, %%%d, %s" % (k, idx[a], idx[b], src2))
    outs = ", ".join('"=&v"(h[%d])' % k for k in range(10))
    ins = ", ".join(['"s"(b26)', '"s"(b25)'] + ['"v"(%s)' % n for n in names])
    body = "\\n\\t".join(lines)
    decl = []
    done = set()
    for n in names:
        kind, i = n.split("_")
        mul = {"f": None, "g": None, "f2": 2, "f4": 4, "g19": 19, "f19": 19, "f38": 38}[kind]
        src = ("g" if kind.startswith("g") else "f") + ".v[%s]" % i
        if kind == "f38" and ("f19_" + i) in names:
            # 2 (19 f): a shift of the 19 f the product needs anyway (VOP2) instead of a second
            # v_mul_lo_u32; the empty asm keeps the compiler from folding it back into 38 f
            decl.append("i32 f19_%s = (i32)(19u * (u32)%s); asm(\"\" : \"+v\"(f19_%s)); const i32 %s = (i32)((u32)f19_%s << 1);"
                        % (i, src, i, n, i))
            done.add("f19_" + i)
        elif n in done:
            continue
        else:
            decl.append("const i32 %s = %s;" % (n, src if mul is None else "(i32)(%du * (u32)%s)" % (mul, src)))
    return """// %s
FE_DEV void %s(%s, i64 h[10]) {
  %s
  const i64 b26 = (i64)1 << 25, b25 = (i64)1 << 24;
  asm("%s"
      : %s
      : %s
      : "vcc");
}
""" % (doc, name, "const fe& f, const fe& g" if "mul" in name else "const fe& f", "\n  ".join(decl), body, outs, ins)


OUT_U = os.path.join(os.path.dirname(HERE), "narwhal_amd", "csrc", "feu_asm.h")
U_MUL = {"f": 1, "g": 1, "f2": 2, "f4": 4, "g19": 19, "f19": 19, "f38": 38}


def emit_u(name, cols, doc):
    """The unsigned, carry-seeded product (fe_u25519.h): column k is one v_mad_u64_u32 chain whose
    first addend is the carry of column k - 1; a 64-bit shift and a mask end it.  One asm statement
    per column (inline asm cannot name the low half of a 64-bit operand, which the mask needs), so
    the whole product is one serial chain -- the layout tools/microbench/mad_chain.hip measured.
    The same text builds for the host and for the bound shadow through the FEU_* macros."""
    mul = "mul" in name
    names = []
    for c in cols:
        for a, b in c:
            for x in (a, b):
                if x not in names:
                    names.append(x)
    body = []
    for n in names:
        kind, i = n.split("_")
        src = ("g" if kind.startswith("g") else "f") + ".v[%s]" % i
        body.append("const FEU_OP %s = FEU_PREP(%du, %s);" % (n, U_MUL[kind], src))
    body.append("feu r; FEU_ACC h;")
    for k, col in enumerate(cols):
        ops = []
        for a, b in col:
            for x in (a, b):
                if x not in ops:
                    ops.append(x)
        idx = {n: 1 + i for i, n in enumerate(ops)}
        lines = []
        for t, (a, b) in enumerate(col):
            src2 = "0" if (k == 0 and t == 0) else "%0"
            lines.append("v_mad_u64_u32 %%0, vcc, %%%d, %%%d, %s" % (idx[a], idx[b], src2))
        w = 25 if k & 1 else 26
        body.append("#if FEU_USE_ASM")
        body.append('asm("%s" : %s : %s : "vcc");' % ("\\n\\t".join(lines), '"=&v"(h)' if k == 0 else '"+v"(h)',
                                                      ", ".join('"v"(%s)' % n for n in ops)))
        body.append("#else")
        if k == 0:
            body.append("h = 0;")
        body.append(" ".join("FEU_MA(h, %s, %s);" % (a, b) for a, b in col))
        body.append("#endif")
        body.append("FEU_COL_END(h); r.v[%d] = (u32)h & %du; h >>= %d;" % (k, (1 << w) - 1, w))
    # the carry out of column 9 re-enters limb 0 with weight 19 (it can pass 2^32: a 64-bit step),
    # and what limb 0 then carries stays on limb 1 as slack
    body.append("h = (FEU_ACC)r.v[0] + h * 19u; FEU_COL_END(h);")
    body.append("r.v[0] = (u32)h & %du; r.v[1] += (u32)(h >> 26);" % ((1 << 26) - 1))
    body.append("return r;")
    return "// %s\nFEU_FN feu %s(%s) {\n  %s\n}\n" % (doc, name, "const feu& f, const feu& g" if mul else "const feu& f",
                                                    "\n  ".join(body))


def main():
    usrc = ["// Generated by tools/gen_fe_asm.py -- do not edit.  Included by fe_u25519.h inside namespace nwc,",
            "// after feu / u32 / u64 and the FEU_* macros (not a standalone header; no include guard, so a",
            "// host test can include it a second time, in a namespace of its own, with the macros of its",
            "// 128-bit bound shadow).",
            emit_u("feu_mul", mul_terms(), "f * g, carried (100 v_mad_u64_u32)"),
            emit_u("feu_sq", sq_terms(False), "f^2, carried (55 v_mad_u64_u32)"),
            emit_u("feu_sq2", sq_terms(True), "2 f^2, carried (55 v_mad_u64_u32)"), ""]
    open(OUT_U, "w").write("\n".join(usrc))
    print("wrote", OUT_U)
    src = ["// Generated by tools/gen_fe_asm.py -- do not edit.  Included by fe25519.h after the",
           "// definitions of fe / i32 / i64 / FE_DEV (not a standalone header).", "#pragma once",
           "namespace nwc {",
           emit("fe_mul_wide_asm", mul_terms(), "h = f * g + column bias (100 v_mad_i64_i32)"),
           emit("fe_sq_wide_asm", sq_terms(False), "h = f^2 + column bias (55 v_mad_i64_i32)"),
           emit("fe_sq2_wide_asm", sq_terms(True), "h = 2 f^2 + column bias (55 v_mad_i64_i32)"),
           "}  // namespace nwc", ""]
    open(OUT, "w").write("\n".join(src))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
