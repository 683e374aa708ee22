"""CPU: the fma form of the Jacobi update is the reference's form, bit for
bit, whenever the guard's condition holds -- and is not above it.

Reference (model.rs:775-793 with reciprocal multiply, R = 1/dx^2 = 1/dy^2 =
2^k):   d = (h * R + v * R) - Rh        three roundings
fma form: d = fma(h + v, R, -Rh)         (h + v) * R is exact below overflow

A small C program (built here with the host compiler, -ffp-contract=off)
evaluates both for R in {2^10, 2^14, 2^24} over a few million random bit
patterns and edge sets (+-0, subnormals, values straddling 2^-126, |h|, |v|
up to just under the guard's limit 2^125 / R -- the march's |h|, |v| <= 2 max
|p'| with max |p'| < 2^123 / R, two binades inside -- and Rh subnormal and
huge), asserts equal bits under the guard and prints a counter-example above
it."""
import os
import shutil
import subprocess

import pytest

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static float f_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t b_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
static int same(float a, float b) { return b_of(a) == b_of(b) || (isnan(a) && isnan(b)); }
static float ref(float h, float v, float R, float Rh) {
    volatile float hz = h * R, vt = v * R;
    volatile float sm = hz + vt;
    return sm - Rh;
}
static float fma_form(float h, float v, float R, float Rh) {
    volatile float t = h + v;
    return fmaf(t, R, -Rh);
}
int main(void) {
    const int ks[3] = {10, 14, 24};
    long checked = 0, bad = 0, above = 0;
    for (int q = 0; q < 3; ++q) {
        const float R = ldexpf(1.0f, ks[q]);
        const float lim = ldexpf(1.0f, 125 - ks[q]);   /* |h|, |v| below it under the guard */
        float edge[64];
        int ne = 0;
        const float e0[] = {0.0f, f_of(1), f_of(0x007FFFFF), f_of(0x00800000), f_of(0x00800001),
                            f_of(0x00400000), ldexpf(1.0f, -126 - ks[q]), ldexpf(1.5f, -127),
                            1.0f, 3.0f, 0.1f, ldexpf(1.0f, -ks[q]), ldexpf(1.75f, -126 + ks[q]),
                            nextafterf(lim, 0.0f), lim * 0.5f, lim * 0.75f, ldexpf(1.0f, 100 - ks[q])};
        for (unsigned i = 0; i < sizeof e0 / sizeof *e0; ++i) { edge[ne++] = e0[i]; edge[ne++] = -e0[i]; }
        float rhe[32];
        int nr = 0;
        const float r0[] = {0.0f, f_of(1), f_of(0x007FFFFF), f_of(0x00800000), 1.0f, 1e-3f,
                            ldexpf(1.0f, 100), ldexpf(1.0f, 126), 3.0e38f, ldexpf(1.25f, -120)};
        for (unsigned i = 0; i < sizeof r0 / sizeof *r0; ++i) { rhe[nr++] = r0[i]; rhe[nr++] = -r0[i]; }
        for (int a = 0; a < ne; ++a)
            for (int b = 0; b < ne; ++b)
                for (int c = 0; c < nr; ++c) {
                    ++checked;
                    if (!same(ref(edge[a], edge[b], R, rhe[c]), fma_form(edge[a], edge[b], R, rhe[c]))) {
                        ++bad;
                        printf("MISMATCH R=2^%d h=%a v=%a Rh=%a\n", ks[q], edge[a], edge[b], rhe[c]);
                    }
                }
        for (long i = 0; i < 2000000; ++i) {
            float h = f_of(rnd()), v = f_of(rnd()), Rh = f_of(rnd());
            if (i & 1) {   /* the small end: subnormal and near-subnormal operands */
                h = f_of((rnd() & 0x80FFFFFFu) | ((rnd() % 40) << 23));
                v = f_of((rnd() & 0x80FFFFFFu) | ((rnd() % 40) << 23));
            }
            if (i % 3 == 0) Rh = f_of((rnd() & 0x80FFFFFFu) | ((rnd() % 30) << 23));
            if (!(fabsf(h) < lim) || !(fabsf(v) < lim) || isnan(Rh)) continue;   /* the guard */
            ++checked;
            if (!same(ref(h, v, R, Rh), fma_form(h, v, R, Rh))) {
                ++bad;
                if (bad < 10) printf("MISMATCH R=2^%d h=%a v=%a Rh=%a\n", ks[q], h, v, Rh);
            }
        }
        /* above the limit the forms part: h R overflows where (h + v) R does not */
        const float h = ldexpf(1.5f, 128 - ks[q]), v = -ldexpf(1.25f, 128 - ks[q]);
        if (!same(ref(h, v, R, 1.0f), fma_form(h, v, R, 1.0f))) {
            ++above;
            printf("COUNTER R=2^%d h=%a v=%a: ref %a fma %a\n", ks[q], h, v, ref(h, v, R, 1.0f),
                   fma_form(h, v, R, 1.0f));
        }
    }
    printf("checked %ld bad %ld above %ld\n", checked, bad, above);
    return bad ? 1 : 0;
}
"""


def test_fma_form_equals_reference_under_the_guard(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler (the oracle's build needs one too)"
    src = tmp_path / "sums_fma.c"
    src.write_text(SRC)
    exe = tmp_path / "sums_fma"
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", str(exe), str(src), "-lm"],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    checked, bad, above = int(last[1]), int(last[3]), int(last[5])
    assert bad == 0 and checked > 3_000_000, last
    assert above >= 1 and "COUNTER" in r.stdout, "no counter-example above the limit: is the guard needed?"
