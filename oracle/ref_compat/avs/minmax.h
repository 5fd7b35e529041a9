/* oracle/ref_compat/avs/minmax.h -- TEST INFRASTRUCTURE ONLY: global min / max / clamp templates under the name the
 * AviSynth+ SDK gives its header of that purpose (see ../avisynth_c.h for why this directory exists). */
#ifndef JINCRESIZE_REF_COMPAT_AVS_MINMAX_H
#define JINCRESIZE_REF_COMPAT_AVS_MINMAX_H

template <typename T>
T min(T v1, T v2) {
    return v1 < v2 ? v1 : v2;
}

template <typename T>
T max(T v1, T v2) {
    return v1 > v2 ? v1 : v2;
}

template <typename T>
T clamp(T n, T lo, T hi) {
    n = n > hi ? hi : n;
    return n < lo ? lo : n;
}

#endif
