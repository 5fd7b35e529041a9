// kernel_framelane_common.inc -- pieces shared by the frame-lane kernels (kernel_framelane.hip: 64 frames per workgroup,
// kernel_framelane_pair.hip: 128 frames per workgroup, two per lane): tile location, per-tile tables, staging, packed stores.
// Included inside namespace jinc { namespace { of a kernel translation unit, after device_common.hpp.


template <typename T>
struct FlPack;  // four horizontally adjacent samples of one frame
template <>
struct FlPack<uint8_t> {
    using type = uint32_t;
};
template <>
struct FlPack<uint16_t> {
    using type = uint2;
};
template <>
struct FlPack<half_t> {
    using type = uint2;
};
template <>
struct FlPack<bf16_t> {
    using type = uint2;
};
template <>
struct FlPack<float> {
    using type = float4;
};

template <typename T>
__device__ __forceinline__ typename FlPack<T>::type fl_pack(const float (&r)[4], float peak) {
    if constexpr (std::is_same_v<T, uint8_t>) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) w = __builtin_amdgcn_cvt_pk_u8_f32(r[i], static_cast<uint32_t>(i), w);
        return w;
    } else if constexpr (std::is_same_v<T, uint16_t>) {
        uint2 w;
        w.x = round_sample(r[0], peak) | (round_sample(r[1], peak) << 16);
        w.y = round_sample(r[2], peak) | (round_sample(r[3], peak) << 16);
        return w;
    } else if constexpr (std::is_same_v<T, half_t>) {
        return make_uint2(round_pair_f16(r[0], r[1]), round_pair_f16(r[2], r[3]));
    } else if constexpr (std::is_same_v<T, bf16_t>) {
        return make_uint2(round_pair_bf16(r[0], r[1]), round_pair_bf16(r[2], r[3]));
    } else {
        return make_float4(r[0], r[1], r[2], r[3]);
    }
}

// Tile of a workgroup and its source footprint (all wave-uniform).
struct FlTile {
    int bx0, by0, bx1, by1;  // output pixels, inclusive
    int tx0, ty0, tw, th;    // source footprint: origin and extent
    int f0, nfg;             // first frame of the group, frames in it (<= frames per workgroup)
};

// block -> tile.  Workgroups are dealt round-robin over the 8 XCDs by linear id; XCD k walks the contiguous run of
// tiles [k*q + min(k, rem), ...) so that the halos shared by neighbouring tiles stay in one L2.  False: padding block.
template <int FPG = 64>  // frames per workgroup
__device__ __forceinline__ bool fl_locate(const FrameLaneArgs& a, int fs, FlTile& t) {
    const DevicePlan& p = a.plan;
    const int ntiles = a.block_begin[4];
    const int q = ntiles / 8, rem = ntiles % 8;
    const int xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
    if (idx >= q + (xcd < rem ? 1 : 0)) return false;
    const int tid = xcd * q + (xcd < rem ? xcd : rem) + idx;
    int r = 0;
    while (r + 1 < a.rects.n && tid >= a.block_begin[r + 1]) ++r;
    const int local = tid - a.block_begin[r];
    const int tcx = local % a.tiles_x[r], tcy = local / a.tiles_x[r];
    const int rx1 = a.rects.x0[r] + a.rects.w[r], ry1 = a.rects.y0[r] + a.rects.h[r];
    t.bx0 = a.rects.x0[r] + (tcx << a.tx_shift), t.by0 = a.rects.y0[r] + (tcy << a.ty_shift);
    t.bx1 = min(t.bx0 + (1 << a.tx_shift), rx1) - 1, t.by1 = min(t.by0 + (1 << a.ty_shift), ry1) - 1;
    t.tx0 = p.col_start[t.bx0], t.ty0 = p.row_start[t.by0];
    t.tw = p.col_start[t.bx1] + fs - t.tx0;  // <= 64 (host: framelane_configure)
    t.th = p.row_start[t.by1] + fs - t.ty0;
    t.f0 = blockIdx.y * FPG;
    t.nfg = min(FPG, a.io.nframes - t.f0);
    return true;
}

// Per-tile tables in LDS: window origins and the coefficient set of every pixel (looked up once per pixel for 64 frames).
__device__ __forceinline__ void fl_tables(const FrameLaneArgs& a, const FlTile& t, int* cs, int* rs, int* sets) {
    const DevicePlan& p = a.plan;
    for (int i = threadIdx.x; i < (1 << a.tx_shift); i += blockDim.x) cs[i] = p.col_start[min(t.bx0 + i, t.bx1)];
    for (int i = threadIdx.x; i < (1 << a.ty_shift); i += blockDim.x) rs[i] = p.row_start[min(t.by0 + i, t.by1)];
    for (int i = threadIdx.x; i < (1 << (a.tx_shift + a.ty_shift)); i += blockDim.x) {
        const int ix = i & ((1 << a.tx_shift) - 1), iy = i >> a.tx_shift;
        const int qx = min(t.bx0 + ix, t.bx1), qy = min(t.by0 + iy, t.by1);
        const int rc = p.row_class[qy], cc = p.col_class[qx];
        int set;
        if (rc < 0)
            set = p.brow_set[static_cast<size_t>(~rc) * p.dst_w + qx];
        else if (cc < 0)
            set = p.bcol_set[static_cast<size_t>(~cc) * p.dst_h + qy];
        else
            set = p.interior_set[rc * p.n_col_classes + cc];
        sets[iy * kFrameLaneMaxTile + ix] = set;
    }
}

// Stages the source footprint of the group's frames in LDS in the source format, one position per source sample of the
// tile and FPG frames per position (PS bytes apart): position (row, col) = row * row_pos + col * col_pos.  Global loads
// run along the columns of one frame (coalesced).  A wave owns the frames wave, wave + nwaves, ...; a batch is UF of its
// frames x US row steps = 16 loads in flight (UF = the frames a wave owns in a full group, so no slot idles: per-frame
// batches of 16 slots kept 10 loads in flight for a tile of 19 rows and went through a wave's frames one memory latency
// after the other).  The frame bases are wave-uniform (scalar registers, one set per batch of frames), a lane adds its
// constant offsets: two vector instructions per row step and one per LDS write (was 6 + 4 scalar + a branch per load:
// staging was 23 of the pair kernel's 149 vector instructions per pixel pair).  Slots past the wave's frames or the tile's
// rows re-read a valid sample (clamped) and are not written.
template <typename T, int PS, int UF, int US>
__device__ __forceinline__ void fl_stage(const FrameLaneArgs& a, const FlTile& t, char* tile, int row_pos, int col_pos, int lane,
                                         int wave, int nwaves) {
    constexpr int SB = static_cast<int>(sizeof(T));
    using Raw = std::conditional_t<sizeof(T) == 4, uint32_t, std::conditional_t<sizeof(T) == 2, uint16_t, uint8_t>>;  // (samples travel as bits, one 32-bit register each)
    const int tw = t.tw, th = t.th;
    const int sh = tw <= 1 ? 0 : 32 - __builtin_clz(static_cast<unsigned>(tw - 1));  // lanes per row = 1 << sh >= tw
    const int lc = lane & ((1 << sh) - 1), lr = lane >> sh, rps = 64 >> sh;
    const int nsteps = (th + rps - 1) >> (6 - sh);
    const int nfw = t.nfg > wave ? (t.nfg - wave + nwaves - 1) / nwaves : 0;  // frames of this wave
    if (lc >= tw || nfw == 0) return;  // (nothing to load or write; the caller's barrier follows)
    const uint32_t pitch = static_cast<uint32_t>(a.io.src_pitch);
    const uint32_t col_off = static_cast<uint32_t>(lc) * SB;
    const uint32_t last_off = col_off + static_cast<uint32_t>(th - 1) * pitch;  // rows past the tile re-read its last row
    const uint32_t off0 = col_off + static_cast<uint32_t>(lr) * pitch, off_step = static_cast<uint32_t>(rps) * pitch;
    const uint32_t lds0 = static_cast<uint32_t>(lc * col_pos + lr * row_pos) * PS + static_cast<uint32_t>(wave) * SB;
    const uint32_t lds_step = static_cast<uint32_t>(rps * row_pos) * PS;
    const bool last_ok = (nsteps - 1) * rps + lr < th;  // only a frame's last step can fall below the tile
    const size_t fstride = static_cast<size_t>(nwaves) * a.io.src_frame_stride;  // between two frames of this wave
    const char* base0 = static_cast<const char*>(a.io.src) + static_cast<size_t>(t.f0 + wave) * a.io.src_frame_stride +
                        static_cast<size_t>(t.ty0) * pitch + static_cast<size_t>(t.tx0) * SB;  // wave-uniform
    for (int k0 = 0; k0 < nfw; k0 += UF) {
        const char* base[UF];
#pragma unroll
        for (int kk = 0; kk < UF; ++kk) base[kk] = base0 + static_cast<size_t>(min(k0 + kk, nfw - 1)) * fstride;
        for (int s0 = 0; s0 < nsteps; s0 += US) {
            uint32_t v[US][UF];
#pragma unroll
            for (int ss = 0; ss < US; ++ss) {
                const uint32_t off = min(off0 + static_cast<uint32_t>(s0 + ss) * off_step, last_off);
#pragma unroll
                for (int kk = 0; kk < UF; ++kk) v[ss][kk] = static_cast<uint32_t>(*reinterpret_cast<const Raw*>(base[kk] + off));
            }
#pragma unroll
            for (int ss = 0; ss < US; ++ss) {
                if (s0 + ss < nsteps && (s0 + ss < nsteps - 1 || last_ok)) {
                    char* l = tile + lds0 + static_cast<uint32_t>(s0 + ss) * lds_step;
#pragma unroll
                    for (int kk = 0; kk < UF; ++kk)
                        if (k0 + kk < nfw)  // wave-uniform
                            *reinterpret_cast<Raw*>(l + static_cast<uint32_t>((k0 + kk) * nwaves) * SB) = static_cast<Raw>(v[ss][kk]);
                }
            }
        }
    }
}

// Stores up to four horizontally adjacent results of a lane's frame: one packed store where the address allows it.
template <typename T>
__device__ __forceinline__ void fl_store4(char* d, const float (&res)[4], int nvx, bool vec, float peak) {
    if (vec) {
        *reinterpret_cast<typename FlPack<T>::type*>(d) = fl_pack<T>(res, peak);
    } else {
#pragma unroll
        for (int xx = 0; xx < 4; ++xx)
            if (xx < nvx) store_sample<T>(reinterpret_cast<T*>(d) + xx, res[xx], peak);
    }
}


// ------------------------------------------------------------------------------------------------
// 8-bit planes, frame-pair form: the packed results of 16 consecutive pixels of a strip are parked in four dwords per
// frame and leave as ONE 16-byte store.  A lane writes to its own frame, so every store instruction walks 64 different
// cache lines whatever its width; one store per four pixels and frame made the store path the kernel's second limit
// (stores switched off, results discarded: 2x forced onto this form 37 -> 64 % of the VALU peak, 1.37x 47 -> 51 %).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fl_park4(uint32_t (&ob)[4], int g, uint32_t v) {  // g wave-uniform: static register indices
    switch (g & 3) {
        case 0: ob[0] = v; break;
        case 1: ob[1] = v; break;
        case 2: ob[2] = v; break;
        default: ob[3] = v; break;
    }
}
// Stores the group of up to 16 pixels starting at byte d (n valid pixels; vec bit 0: dword stores allowed, bit 1: 16-byte).
__device__ __forceinline__ void fl_flush16_u8(const uint32_t (&ob)[4], char* d, int n, int vec) {
    if (n >= 16 && (vec & 2)) {  // wave-uniform
        *reinterpret_cast<uint4*>(d) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
        return;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int m = n - 4 * g;  // pixels of this dword
        if (m >= 4 && (vec & 1)) {
            *reinterpret_cast<uint32_t*>(d + 4 * g) = ob[g];
        } else {
#pragma unroll
            for (int xx = 0; xx < 4; ++xx)
                if (xx < m) reinterpret_cast<uint8_t*>(d + 4 * g)[xx] = static_cast<uint8_t>(ob[g] >> (8 * xx));
        }
    }
}
