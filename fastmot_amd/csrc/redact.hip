// Stage (a) of the redaction path (fastmot_hip.h "Redaction of the frames that leave the GPU"): the cell
// means of every region of a list, in one launch.  Stage (b), the apply, is part of the tile pass of overlay.hip.
//
// A workgroup of 256 threads owns ONE ROW OF CELLS of one region -- which, it finds by bisecting the per-region table of
// cell-row counts -- and walks it in chunks of at most 1024 pixel columns that begin and end on cell borders.  In a chunk
// a thread owns four neighbouring columns, which it sums over the rows in twelve registers; the threads are laid out as
// (rows x quads) with as many quads as the chunk has and the rest of the 256 stacked over the rows, so that a narrow
// region still fills its wavefronts.  The registers go to per-cell sums in LDS (one atomic per run of columns that share
// a cell), and one thread per cell divides by that cell's own pixel count.  A cell's sum is at most 256 * 256 * 255 < 2^24.
//
// Frame rows are 3-byte pixels, so a thread's 12 bytes begin at any alignment: it reads the three or four ALIGNED dwords
// that hold them and shifts; bytes are read singly only for a chunk's last, partial quad and where the fourth dword would
// reach past the frame's end.
//
// Bounds: reads lie in [src, src + 3 W H): columns xs .. xe and rows ya .. yb are inside the region's rectangle clipped to
// the frame.  A cell's index in the chunk is below CHUNK_PX / c <= 512, its word in `means` below the region's offset plus
// its cell count, which the host summed from the same fm_red_grid.
#include "common.h"
#include "redact_pixel.h"

namespace {

constexpr int RWG = 256, CHUNK_PX = 1024, CHUNK_CELLS = CHUNK_PX / 2;

__global__ __launch_bounds__(RWG) void redact_means_kernel(const uint8_t* __restrict__ src, int W, int H,
                                                           const fm_redact_region* __restrict__ regions, int n,
                                                           const int2* __restrict__ tab, uint32_t* __restrict__ means) {
    __shared__ unsigned acc[CHUNK_CELLS * 3];
    const int tid = threadIdx.x, row = blockIdx.x;
    int lo = 0, hi = n;                       // tab[lo].y <= row < tab[hi].y: region lo has this cell row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].y <= row) lo = mid; else hi = mid;
    }
    const fm_redact_region r = regions[lo];
    const FmRedGrid g = fm_red_grid(r, W, H);
    const int c = r.cell, j = g.jmin + (row - tab[lo].y), ncx = g.imax - g.imin + 1;
    if (j > g.jmax) return;                   // (never: the table was made from the same grid)
    int ya;
    const int nrows = fm_red_cell_span(r.y0, c, j, g.cy0, g.cy1, ya), yb = ya + nrows - 1;
    uint32_t* const out = means + (size_t)tab[lo].x + (size_t)(j - g.jmin) * ncx;
    const uint8_t* const end = src + (size_t)W * H * 3;
    const int per_chunk = CHUNK_PX / c;       // 4 .. 512 cells

    for (int ia = g.imin; ia <= g.imax; ia += per_chunk) {
        const int ib = min(ia + per_chunk - 1, g.imax), ncell = ib - ia + 1;
        const int xs = max(r.x0 + ia * c, g.cx0), xe = min(r.x0 + (ib + 1) * c - 1, g.cx1);
        const int nquads = (xe - xs + 4) >> 2;
        int tpr = 1;                          // threads per row: the power of two that holds the quads
        while (tpr < nquads) tpr <<= 1;
        const int step = RWG / tpr;
        for (int k = tid; k < ncell * 3; k += RWG) acc[k] = 0;
        __syncthreads();

        const int x = xs + 4 * (tid & (tpr - 1)), cnt = min(max(xe - x + 1, 0), 4);
        if (cnt > 0) {
            unsigned s[4][3] = {};
            for (int y = ya + tid / tpr; y <= yb; y += step) {
                const uint8_t* const p = src + ((size_t)y * W + x) * 3;
                const uint32_t* const q = reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3);
                const unsigned sh = ((uintptr_t)p & 3u) * 8u;
                uint32_t w0, w1, w2;
                bool wide = cnt == 4 && reinterpret_cast<const uint8_t*>(q) >= src;
                if (wide && sh == 0) {
                    w0 = q[0], w1 = q[1], w2 = q[2];
                } else if (wide && reinterpret_cast<const uint8_t*>(q + 4) <= end) {
                    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
                    w0 = d0 >> sh | d1 << (32u - sh), w1 = d1 >> sh | d2 << (32u - sh), w2 = d2 >> sh | d3 << (32u - sh);
                } else {
                    wide = false;
                    w0 = w1 = w2 = 0;
                }
                if (wide) {
                    s[0][0] += w0 & 255, s[0][1] += (w0 >> 8) & 255, s[0][2] += (w0 >> 16) & 255;
                    s[1][0] += w0 >> 24, s[1][1] += w1 & 255, s[1][2] += (w1 >> 8) & 255;
                    s[2][0] += (w1 >> 16) & 255, s[2][1] += w1 >> 24, s[2][2] += w2 & 255;
                    s[3][0] += (w2 >> 8) & 255, s[3][1] += (w2 >> 16) & 255, s[3][2] += w2 >> 24;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            if (k < cnt) s[k][ch] += p[k * 3 + ch];
                }
            }
            // columns that share a cell leave as one add
            int cell = (x - r.x0) / c - ia, left = r.x0 + (cell + ia + 1) * c - x;      // columns of `cell` from x on
            unsigned run[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < cnt) {
                    if (left == 0) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) atomicAdd(&acc[cell * 3 + ch], run[ch]), run[ch] = 0;
                        ++cell, left = c;
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) run[ch] += s[k][ch];
                    --left;
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) atomicAdd(&acc[cell * 3 + ch], run[ch]);
        }
        __syncthreads();
        for (int k = tid; k < ncell; k += RWG) {
            int xa;
            const unsigned cnt_px = (unsigned)fm_red_cell_span(r.x0, c, ia + k, g.cx0, g.cx1, xa) * (unsigned)nrows;
            out[ia - g.imin + k] = fm_red_mean(acc[k * 3], cnt_px) | fm_red_mean(acc[k * 3 + 1], cnt_px) << 8 | fm_red_mean(acc[k * 3 + 2], cnt_px) << 16;
        }
        __syncthreads();                      // acc is cleared again by the next chunk
    }
}

}  // namespace

// For overlay.hip (fm_frame_render_redacted): the means of `n` regions on the W x H frame `src` -> `means`; tab[k] =
// {first word of region k in means, cell rows of the regions before k}, tab[n].y = `rows`, the launch's workgroups.
int fm_redact_means_launch(hipStream_t s, const uint8_t* src, int W, int H, const fm_redact_region* regions, int n, const int2* tab,
                           int rows, uint32_t* means) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(redact_means_kernel, dim3(rows), dim3(RWG), 0, s, src, W, H, regions, n, tab, means);
    FM_HIP(hipGetLastError());
    return 0;
}
