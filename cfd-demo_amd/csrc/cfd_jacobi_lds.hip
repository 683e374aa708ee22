// cfd_jacobi_lds.hip — kind 5 (cfd_jacobi_lds.h) for T = 1..4, the dispatch
// over T (launch_lds, cfd_internal.h) and the host-side tile geometry every
// kind-5 launch uses (lds_tiles, lds_pad_bytes, lds_sums_grid).
#include "cfd_jacobi_lds.h"

namespace cfd {

// Dynamic LDS added to a launch (bytes) to cap the workgroups the hardware
// places on one CU, so a round of resident waves is spread evenly at a chosen
// occupancy.  Default: 24 KiB on fixed-count launches (MODE 0/1) whose p'
// pair + rhs fit the 256 MiB Infinity Cache: 18 + 24 KiB per 4-wave
// workgroup admits 3 per CU (3 waves per SIMD) where the registers allow 5,
// and the round's 3/5 of the waves each march a 5/3 longer segment (less
// warm-up recompute) on a launch that is VALU- not memory-bound: developed
// 4096^2 cavity 5.60 -> 5.28 us/sweep (profiles/r3/ab_pad3.log).  None on
// HBM-streaming slabs, where more waves in flight pay (8192^2: 23.8 vs 24.5
// us/sweep padded), nor on the speculative launches (ab_pad_parity.log).
// CFD_LDS_PAD=<bytes> forces one value on every launch.
// The test is on the OWNED rows (r4): every slab of the weak-scaling series
// (4096^2, 8192x2048 and 16384x1024, 16.78 M cells, 201 MB) runs the same
// geometry; with the hg ghost rows counted, the 16384x1024 slab (32 ghost rows
// each side, 214 MB) fell past the threshold and ran unpadded while the
// others were padded.  The ghost rows (6 % at C5) still fit the 256 MiB cache.
int lds_pad_bytes(const Geom &g, int mode) {
    static const int forced = [] {
        const char *e = getenv("CFD_LDS_PAD");
        return e ? std::max(0, std::min(64 * 1024, atoi(e))) : -1;
    }();
    if (forced >= 0) return forced;
    constexpr uint64_t kMallResident = 200ull << 20;
    const uint64_t ws = 3ull * (uint64_t)g.nyl * (uint64_t)g.nx * 4u;
    return mode <= 1 && ws <= kMallResident ? 24 * 1024 : 0;
}

// The grid allows the scaled-sum forms (LdsMarch SUMS): reciprocal multiply,
// dx^2 == dy^2 with a power-of-two reciprocal R >= 1 (h * R, v * R exact
// below overflow); CFD_JACOBI_SUMS=0 keeps the reference's form everywhere.
// Read per launch (one getenv) so tests can change it.
bool lds_sums_grid(const Geom &g) {
    const char *ue = getenv("CFD_JACOBI_SUMS");
    int exp2 = 0;
    const float R = g.r_dx_sq;
    const bool pow2 = R >= 1.0f && std::frexp(R, &exp2) == 0.5f;
    return !(ue && atoi(ue) == 0) && g.fastdiv == 1 && g.dx_sq == g.dy_sq && g.r_dx_sq == g.r_dy_sq &&
           pow2;
}

LdsTiles lds_tiles(const Geom &g, int T, int out_lo, int out_hi, int mode, int bpc, bool one_round) {
    LdsTiles t;
    t.pad = lds_pad_bytes(g, mode);
    t.nwc = cdiv(g.nx / 2, lds_outl(T));
    // Segments per wave column.  g.tb_rows > 0: fixed rows per segment.  0
    // (default): as many segments as ONE round of resident waves holds — every
    // SIMD gets its waves at once and the same march length, so no CU waits
    // for a second, partial round — or whole multiples of a round when a round
    // would make segments longer than kMaxRows.
    const int nrows = out_hi - out_lo;
    if (g.tb_rows > 0) {
        t.nseg = cdiv(nrows, g.tb_rows);
    } else {
        constexpr int kMaxRows = 160, kMinRows = 8;
        const int wgs_per_col = std::max(1, g.n_cu * bpc / t.nwc);
        const int per_round = kLdsWaves * wgs_per_col;
        // the persistent launch keeps ONE round whatever the segment length:
        // a tile per resident workgroup, so no tile waits for an owner that is
        // not resident (8192^2: two rounds made half the tiles run by
        // stealing, 274 vs 170 us per block, profiles/r4/prof_r4a)
        const int rounds = one_round ? 1 : std::max(1, cdiv(nrows, (long)per_round * kMaxRows));
        t.nseg = std::max(1, std::min(per_round * rounds, nrows / kMinRows));
    }
    // a segment whose rows reach a global boundary row runs the kCol|kRow
    // path, ~1.45x the VALU work per row of an interior one (r2 wave
    // timeline): it gets ~1/1.45 of the rows
    constexpr int kEdgeWeight = 11;
    const int reach = T + 2;
    t.wlo = out_lo - reach <= 1 - g.j0 ? kEdgeWeight : 16;
    t.whi = out_hi + reach >= g.ny - 2 - g.j0 ? kEdgeWeight : 16;
    return t;
}

void launch_lds(const Geom &g, const Fields &f, int T, int pass, int it, int par, int out_lo,
                int out_hi, uint32_t *rs, hipStream_t s, int mode, int lag) {
    switch (T) {
    case 1: launch_lds_T<1>(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    case 2: launch_lds_T<2>(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    case 3: launch_lds_T<3>(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    case 4: launch_lds_T<4>(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    case 5:
    case 6:
    case 7: launch_lds_t567(g, f, T, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    default: launch_lds_t8(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag); break;
    }
}

}  // namespace cfd
