// gcc_amd/csrc/text_ingest.hip -- edge-list text in HBM -> line ends and int32 records (gfx950): the device form of what
// gcc_amd.ingest.read_lscc does with bytes.split() and np.array(..., dtype=np.int64).
//
// THE TOKEN RULE.  Separators are the six bytes 9, 10, 11, 12, 13 and 32.  A token starts at byte i >= first_byte when text[i] is no
// separator and (i == first_byte or text[i - 1] is a separator); it runs to the next separator or to the end of the text.  Token r,
// counted from first_byte, is field r % fields of record r / fields; only the tokens r < max_tokens are looked at, and only the fields
// below `keep` are converted and stored.  A valid token is at most one '+' or '-' and then one or more ASCII digits; a token of any
// length is classified (a value past 2^31 + 1 stops growing and stays out of range: never a wrapped value).
//
// A tile is GCC_TEXT_TILE_BYTES bytes at an absolute, 16-byte-aligned offset; a lane takes 16 of them in one load.  Bytes below
// first_byte and at or above nbytes count as separators.  Three launches per call, ordered by kernel boundaries (no workgroup waits
// on another):
//   ti_count_kernel    a tile's token starts and newlines.  The byte before a lane's span is the neighbour lane's last, the one
//                      before a wave's span comes through LDS, the one before the tile from one extra load.
//   ti_scan_kernel     one workgroup: the tiles' counts -> int64 exclusive offsets, GCC_TEXT_SCAN_TILES tiles per pass; the totals;
//                      gcc_text_ints' summary words and its SHORT bit.
//   ti_parse_kernel    (gcc_text_ints) the tile's mask again, the rank of every token start in the tile (popcount, wave prefix, wave
//                      offsets in LDS), and every token r < max_tokens checked and -- a kept field -- converted from a copy of the
//                      tile plus a 16-byte halo in LDS: its first 12 bytes in one round trip, the rest of a longer one byte by
//                      byte.  A token that runs past the halo is read on from global memory.
//   ti_select_kernel   (gcc_text_line_ends) a workgroup per query: a binary search over the scanned newline offsets for the tile,
//                      then the rank inside that one tile.
// gcc_text_ints_sep is gcc_text_ints with two knobs, the same kernels: `extra_sep` makes one more byte value a separator (TU's
// A.txt: ','), and `line_records` (ti_parse_kernel<true>) asks that token r be the first on its line exactly when r % fields == 0 --
// the separator run in front of it holds a newline, or it is token 0 -- with the lowest offender's offset in summary[3].
// The only atomics are an integer min (the lowest offending offset, kept as an unsigned word that starts at all ones: -1 as int64)
// and an integer or (the status bits), so every output word is the same for any grid size and any two calls.  No kernel keeps scratch.
#include "task_common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kTile = GCC_TEXT_TILE_BYTES, kLane = 16;
constexpr int kScanTiles = GCC_TEXT_SCAN_TILES, kPer = kScanTiles / kThreads;
constexpr int kFast = 12;                             // bytes of a token that the parse pass reads in one go (sign and ten digits fit)
constexpr int kGrid = 8192;                           // workgroups of a tile kernel: the tiles go round the grid
constexpr int64_t kMaxBytes = (int64_t)1 << 40;       // tile numbers stay int32
constexpr unsigned long long kNone = ~0ull;           // "no such token": -1 as int64
static_assert(kTile == kThreads * kLane, "a lane takes 16 bytes of the tile");
static_assert(kScanTiles == kThreads * kPer && kPer == 4, "a scan pass");

struct TiDev {
    const unsigned char *text;
    long long nbytes, padded, first_byte, max_tokens;
    int fields, keep, tiles;
    unsigned extra_sep;                               // a seventh separator, or 256: no byte
    int line_records;                                 // gcc_text_ints_sep: records follow lines
    int32_t *tile_tok, *tile_nl;                      // per tile: token starts, newlines
    long long *tok_off, *nl_off, *totals;             // their exclusive prefixes; totals[0 .. 1]
    int32_t *out;
    unsigned long long *summary;                      // gcc_text_ints: [4]; NULL for gcc_text_line_ends
    int32_t *status;
    long long lines[GCC_TEXT_MAX_QUERIES];
    int num_lines;
    long long *ends;
};

__device__ __forceinline__ bool is_sep(unsigned c, unsigned extra) { return c - 9u < 5u || c == 32u || c == extra; }

// a lane's 16 bytes of a tile: the bytes themselves, and one bit per byte for a token start and for a newline
struct Span {
    uint4 raw;
    unsigned starts, nl;
};

// every thread of the workgroup calls (one barrier inside); wave_last: kWaves words of LDS that the caller leaves alone until its
// next barrier
__device__ __forceinline__ Span tile_span(const TiDev &a, long long base, unsigned *wave_last)
{
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const long long p0 = base + (long long)tid * kLane;
    Span s;
    s.raw = make_uint4(0u, 0u, 0u, 0u);
    if (p0 < a.padded) s.raw = *reinterpret_cast<const uint4 *>(a.text + p0);
    const long long lo64 = a.first_byte - p0, hi64 = a.nbytes - p0;
    const int lo = lo64 < 0 ? 0 : lo64 > kLane ? kLane : (int)lo64, hi = hi64 < 0 ? 0 : hi64 > kLane ? kLane : (int)hi64;
    const unsigned valid = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    const unsigned w[4] = {s.raw.x, s.raw.y, s.raw.z, s.raw.w};
    unsigned ns = 0, nl = 0;
#pragma unroll
    for (int j = 0; j < kLane; ++j) {
        const unsigned c = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        ns |= (is_sep(c, a.extra_sep) ? 0u : 1u) << j;
        nl |= (c == 10u ? 1u : 0u) << j;
    }
    ns &= valid;
    s.nl = nl & valid;
    const unsigned last = ns >> (kLane - 1);
    if (lane == 63) wave_last[wv] = last;
    unsigned before = wave_shfl_up(last, 1);
    __syncthreads();
    if (lane == 0) {
        if (wv > 0) before = wave_last[wv - 1];
        else before = (p0 > a.first_byte && p0 <= a.nbytes) ? (is_sep(a.text[p0 - 1], a.extra_sep) ? 0u : 1u) : 0u;
    }
    s.starts = ns & ~((ns << 1) | before);
    return s;
}

// exclusive prefix of (x, y) over the workgroup in thread order, and the totals; red: [2][kWaves] of LDS
__device__ __forceinline__ void block_scan2(int x, int y, int &ex, int &ey, int &tx, int &ty, int (*red)[kWaves])
{
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    const int ix = wave_scan_incl(x), iy = wave_scan_incl(y);
    if (lane == 63) {
        red[0][wv] = ix;
        red[1][wv] = iy;
    }
    __syncthreads();
    int bx = 0, by = 0;
    tx = ty = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wv) {
            bx += red[0][w];
            by += red[1][w];
        }
        tx += red[0][w];
        ty += red[1][w];
    }
    __syncthreads();
    ex = bx + ix - x;
    ey = by + iy - y;
}

__global__ __launch_bounds__(kThreads) void ti_count_kernel(TiDev a)
{
    __shared__ unsigned wave_last[kWaves];
    __shared__ int red[2][kWaves];
    for (int t = (int)blockIdx.x; t < a.tiles; t += (int)gridDim.x) {
        const Span s = tile_span(a, (long long)t * kTile, wave_last);
        int ex, ey, tx, ty;
        block_scan2(__builtin_popcount(s.starts), __builtin_popcount(s.nl), ex, ey, tx, ty, red);
        if (threadIdx.x == 0) {
            a.tile_tok[t] = tx;
            a.tile_nl[t] = ty;
        }
    }
}

// one workgroup: a thread takes kPer consecutive tiles of a pass (a pass holds at most kScanTiles * kTile / 2 starts: int32 will do)
__global__ __launch_bounds__(kThreads) void ti_scan_kernel(TiDev a)
{
    __shared__ int red[2][kWaves];
    long long ca = 0, cb = 0;
    for (int base = 0; base < a.tiles; base += kScanTiles) {
        const int t0 = base + (int)threadIdx.x * kPer;
        int x[kPer], y[kPer], sx = 0, sy = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            x[k] = t0 + k < a.tiles ? a.tile_tok[t0 + k] : 0;
            y[k] = t0 + k < a.tiles ? a.tile_nl[t0 + k] : 0;
            sx += x[k];
            sy += y[k];
        }
        int ex, ey, tx, ty;
        block_scan2(sx, sy, ex, ey, tx, ty, red);
        long long oa = ca + ex, ob = cb + ey;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (t0 + k < a.tiles) {
                a.tok_off[t0 + k] = oa;
                a.nl_off[t0 + k] = ob;
            }
            oa += x[k];
            ob += y[k];
        }
        ca += tx;
        cb += ty;
    }
    if (threadIdx.x == 0) {
        a.totals[0] = ca;
        a.totals[1] = cb;
        if (a.summary) {
            a.summary[0] = (unsigned long long)ca;
            a.summary[1] = kNone;
            a.summary[2] = kNone;
            a.summary[3] = a.line_records ? kNone : 0;
            if (ca < a.max_tokens) atomicOr(a.status, (int32_t)GCC_STATUS_TEXT_SHORT);
        }
    }
}

// x / fields and x % fields for the four record widths, each a division by a constant (a 64-bit division by a run-time value is a
// loop of a hundred instructions; the tile's first token pays it once, a token never)
template <class U> __device__ __forceinline__ void div_fields(U x, int fields, U &q, unsigned &r)
{
    switch (fields) {
    case 1: q = x; break;
    case 2: q = x / 2u; break;
    case 3: q = x / 3u; break;
    default: q = x / 4u; break;
    }
    r = (unsigned)(x - q * (U)fields);
}

// kLines: records follow lines (gcc_text_ints_sep's line_records)
template <bool kLines> __global__ __launch_bounds__(kThreads) void ti_parse_kernel(TiDev a)
{
    __shared__ unsigned wave_last[kWaves];
    __shared__ int red[2][kWaves];
    __shared__ uint4 tile[kThreads + 1];              // the tile and a halo of one lane's bytes
    const unsigned *words = reinterpret_cast<const unsigned *>(tile);
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(tile);
    const int tid = (int)threadIdx.x;
    for (int t = (int)blockIdx.x; t < a.tiles; t += (int)gridDim.x) {
        const long long base = (long long)t * kTile, tok0 = a.tok_off[t];
        if (tok0 >= a.max_tokens) continue;           // (the whole workgroup: nothing of this tile is looked at)
        const Span s = tile_span(a, base, wave_last);
        tile[tid] = s.raw;
        if (tid == 0) {
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (base + kTile < a.padded) h = *reinterpret_cast<const uint4 *>(a.text + base + kTile);
            tile[kThreads] = h;
        }
        int ex, ey, tx, ty;
        block_scan2(__builtin_popcount(s.starts), 0, ex, ey, tx, ty, red);         // (its barriers publish the tile)
        unsigned long long rec0;
        unsigned f0;
        div_fields((unsigned long long)tok0, a.fields, rec0, f0);
        unsigned long long min_bad = kNone, min_range = kNone, min_shape = kNone;
        int bits = 0;
        unsigned rank = (unsigned)ex;
        for (unsigned left = s.starts; left; left &= left - 1, ++rank) {
            if (tok0 + rank >= a.max_tokens) break;
            const int at = tid * kLane + __builtin_ctz(left);      // the token's first byte, within the tile
            const long long off = base + at;
            unsigned q, field;
            div_fields(f0 + rank, a.fields, q, field);
            // bytes [at, stop) of the LDS copy belong to the text; past them the token is read from global memory
            const long long room = a.nbytes - base;
            const int stop = room < kTile + kLane ? (int)room : kTile + kLane;
            unsigned v = 0;                           // the value while it is below 2^31 + 2; `big`: it went past that
            bool bad = false, big = false, neg = false, open = true;
            int digits = 0;
            auto step = [&](unsigned c, bool first) {                   // one byte of the token
                if (first && (c == '-' || c == '+')) {
                    neg = c == '-';
                    return;
                }
                if (is_sep(c, a.extra_sep)) {
                    open = false;
                    return;
                }
                const unsigned d = c - '0';
                if (d > 9u) {
                    bad = true;
                    open = false;
                    return;
                }
                digits = 1;
                if (v > 214748364u) big = true;       // (ten times that and any digit is past 2^31)
                else v = v * 10u + d;
            };
            int i = at;
            if (at + kFast <= stop) {                 // the token's first kFast bytes in one round trip: four words, shifted into place
                const int w0 = at >> 2, sh = 8 * (at & 3);
                const unsigned long long x0 = words[w0], x1 = words[w0 + 1], x2 = words[w0 + 2], x3 = words[w0 + 3];
                const unsigned b[3] = {(unsigned)(((x1 << 32) | x0) >> sh), (unsigned)(((x2 << 32) | x1) >> sh), (unsigned)(((x3 << 32) | x2) >> sh)};
#pragma unroll
                for (int k = 0; k < kFast; ++k)
                    if (open) step((b[k >> 2] >> (8 * (k & 3))) & 255u, k == 0);
                i = at + kFast;
            }
            while (open) {                            // the text's last bytes, and what a token has beyond kFast bytes
                unsigned c;
                if (i < stop) c = bytes[i];
                else if (base + i < a.nbytes) c = a.text[base + i];
                else break;
                step(c, i == at);
                ++i;
            }
            bad = bad || !digits;
            if (bad) {
                bits |= GCC_STATUS_TEXT_NOT_INTEGER;
                min_bad = (unsigned long long)off < min_bad ? (unsigned long long)off : min_bad;
            }
            if ((int)field >= a.keep) continue;
            const bool fits = !big && v <= (neg ? 0x80000000u : 0x7FFFFFFFu);
            if (!bad && !fits) {
                bits |= GCC_STATUS_TEXT_INT32_RANGE;
                min_range = (unsigned long long)off < min_range ? (unsigned long long)off : min_range;
            }
            const unsigned value = neg ? 0u - v : v;
            a.out[(long long)(rec0 + q) * a.keep + field] = (!bad && fits) ? (int32_t)value : 0;
        }
        if (kLines) {
            // a loop of its own (inside the parse loop it costs that loop scalar registers).  First on its line: it is token 0, or
            // the separator run in front of it (which ends at the token before it, at or above first_byte) holds a newline
            rank = (unsigned)ex;
            for (unsigned left = s.starts; left; left &= left - 1, ++rank) {
                if (tok0 + rank >= a.max_tokens) break;
                const long long off = base + tid * kLane + __builtin_ctz(left);
                unsigned q, field;
                div_fields(f0 + rank, a.fields, q, field);
                bool first = tok0 + rank == 0;
                if (!first) {
                    long long p = off - 1;
                    unsigned c = a.text[p];
                    while (c != 10u && is_sep(c, a.extra_sep) && p > a.first_byte) c = a.text[--p];
                    first = c == 10u;
                }
                if (first != (field == 0u)) {
                    bits |= GCC_STATUS_TEXT_LINE_SHAPE;
                    min_shape = (unsigned long long)off < min_shape ? (unsigned long long)off : min_shape;
                }
            }
        }
        if (bits) atomicOr(a.status, (int32_t)bits);
        if (min_bad != kNone) atomicMin(&a.summary[1], min_bad);
        if (min_range != kNone) atomicMin(&a.summary[2], min_range);
        if (kLines && min_shape != kNone) atomicMin(&a.summary[3], min_shape);
        __syncthreads();                              // (the next tile overwrites the copy)
    }
}

// a workgroup per query; workgroup 0 also writes the newline total behind the answers
__global__ __launch_bounds__(kThreads) void ti_select_kernel(TiDev a)
{
    __shared__ unsigned wave_last[kWaves];
    __shared__ int red[2][kWaves];
    const int qi = (int)blockIdx.x;
    const long long total = a.totals[1];
    if (qi == 0 && threadIdx.x == 0) a.ends[a.num_lines] = total;
    if (qi >= a.num_lines) return;
    const long long want = a.lines[qi];
    if (want < 0 || want >= total) {
        if (threadIdx.x == 0) a.ends[qi] = -1;
        return;
    }
    int lo = 0, hi = a.tiles;                         // the last tile whose offset is <= want (nl_off[0] == 0)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.nl_off[mid] <= want) lo = mid;
        else hi = mid;
    }
    const long long base = (long long)lo * kTile;
    const Span s = tile_span(a, base, wave_last);
    const int need = (int)(want - a.nl_off[lo]), cnt = __builtin_popcount(s.nl);
    int ex, ey, tx, ty;
    block_scan2(cnt, 0, ex, ey, tx, ty, red);
    if (need >= ex && need < ex + cnt) {
        unsigned left = s.nl;
        for (int k = ex; k < need; ++k) left &= left - 1;
        a.ends[qi] = base + (long long)threadIdx.x * kLane + __builtin_ctz(left);
    }
}

// ---------------------------------------------------------------- host
struct Plan {
    int64_t off_tile_tok, off_tile_nl, off_tok_off, off_nl_off, off_totals, total;
    int32_t tiles;
};

int check_text(const char *who, int64_t nbytes)
{
    if (nbytes < 1 || nbytes > kMaxBytes) {
        snprintf(g_err, kErrLen, "%s: nbytes %lld outside 1..2^40", who, (long long)nbytes);
        return -2;
    }
    return 0;
}

Plan make_plan(int64_t nbytes)
{
    Plan p;
    p.tiles = (int32_t)((nbytes + kTile - 1) / kTile);
    Carve cv;
    p.off_tile_tok = cv.take((int64_t)p.tiles * 4);
    p.off_tile_nl = cv.take((int64_t)p.tiles * 4);
    p.off_tok_off = cv.take((int64_t)p.tiles * 8);
    p.off_nl_off = cv.take((int64_t)p.tiles * 8);
    p.off_totals = cv.take(16);
    p.total = cv.total();
    return p;
}

// the text's own checks: its address, its alignment, and a capacity of nbytes rounded up to 16
int check_buffer(const char *who, const void *text, int64_t nbytes, int64_t capacity)
{
    const int rc = null_member(who, {{text, "text"}});
    if (rc) return rc;
    const int64_t padded = (nbytes + kLane - 1) / kLane * kLane;
    if (capacity < padded) {
        snprintf(g_err, kErrLen, "%s: capacity %lld is less than nbytes %lld rounded up to 16 (%lld): the kernels load 16 bytes at a time", who,
                 (long long)capacity, (long long)nbytes, (long long)padded);
        return -2;
    }
    if (((uintptr_t)text & 15) != 0) {
        snprintf(g_err, kErrLen, "%s: text must be aligned to 16 bytes", who);
        return -9;
    }
    return 0;
}

TiDev bind(const Plan &pl, void *workspace, const uint8_t *text, int64_t nbytes)
{
    TiDev d = TiDev();
    d.text = text;
    d.nbytes = nbytes;
    d.padded = (nbytes + kLane - 1) / kLane * kLane;
    d.fields = d.keep = 1;
    d.extra_sep = 256u;
    d.tiles = pl.tiles;
    d.tile_tok = ws_at<int32_t>(workspace, pl.off_tile_tok);
    d.tile_nl = ws_at<int32_t>(workspace, pl.off_tile_nl);
    d.tok_off = ws_at<long long>(workspace, pl.off_tok_off);
    d.nl_off = ws_at<long long>(workspace, pl.off_nl_off);
    d.totals = ws_at<long long>(workspace, pl.off_totals);
    return d;
}

int tile_grid(const Plan &pl) { return pl.tiles < kGrid ? pl.tiles : kGrid; }

int run_ints(const char *who, const gcc_text_ints_args *h, int32_t extra_sep, int32_t line_records, void *workspace, int64_t workspace_bytes,
             int32_t *status, void *stream)
{
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_text(who, h->nbytes))) return rc;
    if (h->first_byte < 0 || h->first_byte > h->nbytes) {
        snprintf(g_err, kErrLen, "%s: first_byte %lld outside [0, nbytes = %lld]", who, (long long)h->first_byte, (long long)h->nbytes);
        return -2;
    }
    if (h->fields < 1 || h->fields > 4 || h->keep < 1 || h->keep > h->fields) {
        snprintf(g_err, kErrLen, "%s: fields %d / keep %d: 1 <= keep <= fields <= 4", who, (int)h->fields, (int)h->keep);
        return -2;
    }
    if (h->max_tokens < 0 || h->max_tokens % h->fields != 0) {
        snprintf(g_err, kErrLen, "%s: max_tokens %lld is not a multiple of fields %d", who, (long long)h->max_tokens, (int)h->fields);
        return -2;
    }
    // (the quotient first: max_tokens * keep may not fit int64)
    if (h->max_tokens / h->fields > (int64_t)INT32_MAX / h->keep) {
        snprintf(g_err, kErrLen, "%s: max_tokens %lld / fields %d * keep %d: the words stored must stay below 2^31", who, (long long)h->max_tokens,
                 (int)h->fields, (int)h->keep);
        return -2;
    }
    if ((rc = check_buffer(who, h->text, h->nbytes, h->capacity))) return rc;
    if ((rc = null_member(who, {{status, "status"}, {h->out, "out", h->max_tokens > 0}, {h->summary, "summary"}}))) return rc;
    const Plan pl = make_plan(h->nbytes);
    if ((rc = check_workspace(who, "gcc_text_ints_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    TiDev d = bind(pl, workspace, h->text, h->nbytes);
    d.first_byte = h->first_byte;
    d.max_tokens = h->max_tokens;
    d.fields = h->fields;
    d.keep = h->keep;
    d.out = h->out;
    d.summary = reinterpret_cast<unsigned long long *>(h->summary);
    d.status = status;
    d.extra_sep = extra_sep ? (unsigned)extra_sep : 256u;
    d.line_records = line_records;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ti_count_kernel, dim3(tile_grid(pl)), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(ti_scan_kernel, dim3(1), dim3(kThreads), 0, s, d);
    if (h->max_tokens > 0 && line_records) hipLaunchKernelGGL(ti_parse_kernel<true>, dim3(tile_grid(pl)), dim3(kThreads), 0, s, d);
    else if (h->max_tokens > 0) hipLaunchKernelGGL(ti_parse_kernel<false>, dim3(tile_grid(pl)), dim3(kThreads), 0, s, d);
    return launched();
}

}  // namespace

extern "C" {

int64_t gcc_text_line_ends_workspace_bytes(int64_t nbytes)
{
    const int rc = check_text("gcc_text_line_ends_workspace_bytes", nbytes);
    if (rc) return rc;
    return make_plan(nbytes).total;
}

int64_t gcc_text_ints_workspace_bytes(int64_t nbytes)
{
    const int rc = check_text("gcc_text_ints_workspace_bytes", nbytes);
    if (rc) return rc;
    return make_plan(nbytes).total;
}

int32_t gcc_text_line_ends(const gcc_text_line_ends_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_text_line_ends";
    (void)status;                                     // (the call sets no bit: a status word is accepted and left alone)
    int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    if ((rc = check_text(who, h->nbytes))) return rc;
    if (h->num_lines < 0 || h->num_lines > GCC_TEXT_MAX_QUERIES) {
        snprintf(g_err, kErrLen, "%s: num_lines %d outside 0..%d", who, (int)h->num_lines, GCC_TEXT_MAX_QUERIES);
        return -2;
    }
    if ((rc = check_buffer(who, h->text, h->nbytes, h->capacity))) return rc;
    if ((rc = null_member(who, {{h->lines, "lines", h->num_lines > 0}, {h->ends, "ends"}}))) return rc;
    const Plan pl = make_plan(h->nbytes);
    if ((rc = check_workspace(who, "gcc_text_line_ends_workspace_bytes", workspace, workspace_bytes, pl.total))) return rc;
    TiDev d = bind(pl, workspace, h->text, h->nbytes);
    d.num_lines = h->num_lines;
    for (int i = 0; i < h->num_lines; ++i) d.lines[i] = h->lines[i];
    d.ends = reinterpret_cast<long long *>(h->ends);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ti_count_kernel, dim3(tile_grid(pl)), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(ti_scan_kernel, dim3(1), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(ti_select_kernel, dim3(h->num_lines > 0 ? h->num_lines : 1), dim3(kThreads), 0, s, d);
    return launched();
}

int32_t gcc_text_ints(const gcc_text_ints_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    return run_ints("gcc_text_ints", h, 0, 0, workspace, workspace_bytes, status, stream);
}

int32_t gcc_text_ints_sep(const gcc_text_ints_sep_args *h, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream)
{
    const char *who = "gcc_text_ints_sep";
    const int rc = null_member(who, {{h, "args"}});
    if (rc) return rc;
    const int32_t c = h->extra_sep;
    if (c < 0 || c > 255 || (c >= 9 && c <= 13) || c == 32 || (c >= '0' && c <= '9') || c == '+' || c == '-') {
        snprintf(g_err, kErrLen, "%s: extra_sep %d: 0, or a byte 1..255 that is no separator, digit or sign", who, (int)c);
        return -2;
    }
    if (h->line_records != 0 && h->line_records != 1) {
        snprintf(g_err, kErrLen, "%s: line_records %d is neither 0 nor 1", who, (int)h->line_records);
        return -2;
    }
    return run_ints(who, &h->ints, c, h->line_records, workspace, workspace_bytes, status, stream);
}

}  // extern "C"
