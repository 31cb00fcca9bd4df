// seds_host.hpp -- the host side that iso_unit.hip and sed_unit.hip share: validation of the
// table, its columns and the networks (the messages name the table: "isochrone" / "track"), the
// fill of the device table struct, the compiled network widths and the LDS they need.  Needs
// host.hpp (fail, BandCounts).
#pragma once

#include "host.hpp"
#include "seds_common.hpp"

namespace {

using NetWidths = BandCounts<8, 16, 32, 64>;        // the HP of k_iso_nn / k_sed_nn_fit

// The compiled width that holds a first layer of h1 units; -1: none.
inline int nn_hp(int h1) {
    for (int hp : {8, 16, 32, 64})
        if (h1 <= hp) return hp;
    return -1;
}

// LDS of a network kernel: w1 (HP, 6) | b1 (HP) | w2 (h2, HP) | b2 (h2) | w3 (h2) | b3, then
// what the kernel keeps behind the weights.
inline size_t nn_lds_bytes(int hp, int h2, size_t extra_doubles) {
    return sizeof(double) * ((size_t)hp * 7 + (size_t)h2 * hp + 2 * (size_t)h2 + 1 + extra_doubles);
}

// 0, or the error of a table (four axes of nax[d] nodes, npred predictions) or of one of the six
// columns idx[] the kernels read.
inline int seds_check_table(const char *noun, const int nax[4], int npred, const int idx[6]) {
    int64_t ntab = 1;
    for (int d = 0; d < 4; d++) {
        if (nax[d] < 2 || nax[d] > (1 << 20))
            return fail(BRUTUS_EINVAL, "bad %s table (axes %d x %d x %d x %d, each needs 2 nodes or more)", noun,
                        nax[0], nax[1], nax[2], nax[3]);
        ntab *= nax[d];
    }
    if (npred < 1 || npred > SEDS_MAX_PRED || ntab * npred >= ((int64_t)1 << 40))
        return fail(BRUTUS_EINVAL, "bad %s table (npred=%d, at most %d)", noun, npred, SEDS_MAX_PRED);
    for (int k = 0; k < 6; k++)
        if (idx[k] < 0 || idx[k] >= npred)
            return fail(BRUTUS_EINVAL, "bad %s prediction column %d (npred=%d)", noun, idx[k], npred);
    return 0;
}

// 0, or the error of a network that no compiled width or no LDS holds.
inline int nn_check(int h1, int h2, size_t extra_doubles) {
    const int hp = nn_hp(h1);
    if (h1 < 1 || hp < 0 || h2 < 1 || nn_lds_bytes(hp, h2, extra_doubles) > 64 * 1024)
        return fail(BRUTUS_EINVAL, "bad network (h1=%d, at most %d; h2=%d; at most 64 KiB of weights per filter)",
                    h1, SEDS_MAX_H1, h2);
    return 0;
}

// The table struct of a checked table: d_axes holds the four axes end to end, idx[] the columns
// in the order of the struct's fields.
inline SedsTable seds_table(const double *d_table, const double *d_axes, const int nax[4], int npred,
                            const int idx[6]) {
    SedsTable T;
    T.tab = d_table;
    for (int d = 0; d < 4; d++) {
        T.ax[d] = d_axes;
        T.n[d] = nax[d];
        d_axes += nax[d];
    }
    T.npred = npred;
    T.i_first = idx[0];
    T.i_logl = idx[1];
    T.i_logt = idx[2];
    T.i_logg = idx[3];
    T.i_feh_surf = idx[4];
    T.i_afe_surf = idx[5];
    return T;
}

// The parameters of the empirical corrections into an IsoCall / a SedCall.
template <class Call>
inline void seds_corr(Call &c, const double corr[4]) {
    c.dtdm = corr[0];
    c.drdm = corr[1];
    c.msto_smooth = corr[2];
    c.feh_scale = corr[3];
}

}  // namespace
