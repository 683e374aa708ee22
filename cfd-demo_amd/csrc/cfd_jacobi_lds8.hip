// cfd_jacobi_lds8.hip — kind 5 (cfd_jacobi_lds.h) for T = 8, the default
// launch of the solve, and the geometry report of its two forms.
#include "cfd_jacobi_lds.h"

namespace cfd {

void launch_lds_t8(const Geom &g, const Fields &f, int pass, int par, int it, int out_lo, int out_hi,
                   uint32_t *rs, int mode, hipStream_t s, int lag) {
    launch_lds_T<8>(g, f, pass, par, it, out_lo, out_hi, rs, mode, s, lag);
}

void lds_geometry8(const Geom &g, int out_lo, int out_hi, bool persist, int *pad, int *occ, int *nwc,
                   int *nseg) {
    const int pd = lds_pad_bytes(g, 0);
    const int o = persist ? persist_blocks_per_cu8(g, pd)
                          : with_fastdiv(g.fastdiv, [&](auto F) { return lds_blocks_per_cu<8, F(), 0>(pd); });
    const LdsTiles t = lds_tiles(g, 8, out_lo, out_hi, 0, o, persist);
    if (pad) *pad = t.pad;
    if (occ) *occ = o;
    if (nwc) *nwc = t.nwc;
    if (nseg) *nseg = t.nseg;
}

}  // namespace cfd
