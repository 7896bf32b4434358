// How an entry point that goes from planes to planes reaches a host caller's planes: column windows that fit
// the scratch cap, and per window a cursor over one scratch block that hands every plane to the kernels -- a device plane as it is,
// a host plane staged at the window's width -- and brings the staged outputs back.  Everything is local to the including unit.
#pragma once
#include "engine.h"

namespace {

constexpr int64_t kNoWindowCap = INT64_MAX;
constexpr int kMaxStagedOut = 16;

// The window plan: WW columns a window, of a call of W columns that stages per_col bytes a column (0: nothing is staged, and no
// block is obtained), at most `cap` columns; the block holds one window's staged planes.
struct StageWindows {
    int64_t WW = 0;
    unsigned char *block = nullptr;
};
inline int plan_stage_windows(illico_ctx *c, int64_t W, size_t per_col, int64_t cap, const char *scratch_name, StageWindows *out) {
    out->WW = std::min<int64_t>(W, cap);
    if (!per_col) return ILLICO_OK;
    out->WW = std::max<int64_t>(1, std::min<int64_t>(out->WW, (int64_t)((size_t)std::max<int64_t>(c->scratch_bytes, 1) / per_col)));
    return scratch(c, scratch_name, (size_t)out->WW * per_col + 8 * kMaxStagedOut, &out->block); // (a 4-byte plane is padded to 8 bytes)
}

// [rows][w] elements of esz bytes between two pitches (in elements).  Enqueued, not awaited.
inline int copy_plane(illico_ctx *c, void *dst, int64_t dst_ld, const void *src, int64_t src_ld, int64_t rows, int64_t w, size_t esz, hipMemcpyKind kind) {
    if (rows == 1) HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)w * esz, kind, c->stream));
    else HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dst_ld * esz, src, (size_t)src_ld * esz, (size_t)w * esz, (size_t)rows, kind, c->stream));
    return ILLICO_OK;
}

// The cursor of one window, columns [w0, w0 + wn) of the caller's planes.  in() and out() return the plane as the kernels take it,
// at the pitch pitch() states: a device plane at column w0 with its own pitch; a host plane staged at pitch wn, where the cursor
// stands; a null plane null, taking no room.  The first error sticks in `rc` (later calls do nothing) and finish() returns it.
struct PlaneStage {
    illico_ctx *c;
    unsigned char *at; // the cursor
    int64_t w0, wn;
    int rc = ILLICO_OK;
    bool staged = false;
    struct Down {
        void *host;
        const void *dev;
        int64_t host_ld, rows;
        size_t esz;
    } down[kMaxStagedOut];
    int n_down = 0;

    PlaneStage(illico_ctx *c_, void *block, int64_t w0_, int64_t wn_) : c(c_), at((unsigned char *)block), w0(w0_), wn(wn_) {}

    int64_t pitch(int64_t host_ld, bool on_dev) const { return on_dev ? host_ld : wn; }
    void *rest() const { return at; } // what follows the staged planes is the unit's own

    template <typename T> const T *in(const T *plane, int64_t host_ld, int64_t rows, bool on_dev) {
        if (!plane || rc) return nullptr;
        if (on_dev) return plane + w0;
        T *d = take<T>(rows);
        rc = copy_plane(c, d, wn, plane + w0, host_ld, rows, wn, sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    // a host plane comes back in finish(); with `preload` the caller's contents go up first, so that the columns the kernels leave
    // (skipped, flagged) come back as they were
    template <typename T> T *out(T *plane, int64_t host_ld, int64_t rows, bool on_dev, bool preload) {
        if (!plane || rc) return nullptr;
        if (on_dev) return plane + w0;
        if (n_down == kMaxStagedOut) { rc = fail(c, ILLICO_ERR_ARG, "more than %d staged output planes", kMaxStagedOut); return nullptr; }
        T *d = take<T>(rows);
        down[n_down++] = Down{plane + w0, d, host_ld, rows, sizeof(T)};
        if (preload) rc = copy_plane(c, d, wn, plane + w0, host_ld, rows, wn, sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    // the staged outputs go down; the stream is awaited iff this window staged anything (the block is reused by the next window, and
    // host planes are complete on return)
    int finish() {
        for (int k = 0; k < n_down && !rc; ++k)
            rc = copy_plane(c, down[k].host, down[k].host_ld, down[k].dev, wn, down[k].rows, wn, down[k].esz, hipMemcpyDeviceToHost);
        if (!rc && staged) HIPCHK(c, hipStreamSynchronize(c->stream));
        return rc;
    }

private:
    template <typename T> T *take(int64_t rows) {
        static_assert(sizeof(T) == 4 || sizeof(T) == 8, "planes hold 4-byte or 8-byte elements");
        T *p = (T *)at;
        at += ((size_t)rows * wn * sizeof(T) + 7) & ~(size_t)7;
        staged = true;
        return p;
    }
};

} // namespace
