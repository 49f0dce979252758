/* mcd_host.c -- host-side helper of the CSV writer (plain C, no GPU): numpy's str() of a 1-D float32 row.
 *
 * The drivers' CSV (describe_og_neurons.py:112-116 / describe_broad_neurons.py:112-116) stores the 10 similarities
 * of a neuron as str(np.ndarray): numpy's array2string, i.e. per element the SHORTEST digit string that identifies
 * the float32 (Dragon4, unique=True) cut at 8 fractional digits, padded to common widths, wrapped at 75 columns.
 * At 9216 neurons that is 92 160 Dragon4 calls from Python: 0.1 s, 170x the whole HIP core.  This file produces the
 * same characters for the plain regime (finite, 1e-4 <= |x| < 2^24, max/min <= 999) with exact double arithmetic:
 * for such x and d <= 8, x*10^d and the rounding-interval ends (x +- half the gap to the neighbouring float32)*10^d
 * are exact doubles (<= 44 significant bits), so Dragon4's stopping rule -- stop at the first digit position where
 * the truncated or the incremented digit string lies strictly inside the interval, then round as it does -- is a few
 * comparisons.  Rows outside the regime return -1 and are formatted by numpy itself.
 * tests/test_host_logic_cpu.py compares the two character for character on random rows.
 *
 * Further down: the container half of include/mcd_cache.h (the activation-cache files written in pieces, with the zip CRC-32),
 * tested by tests/test_cache_stream_cpu.py. */
#define _POSIX_C_SOURCE 200809L   /* pwrite */
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static const double P10[9] = {1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8};
static const uint64_t I10[9] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull};

static int ndigits(uint64_t v) {
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

/* |v| -> integer part, fractional digits F with d of them (trailing zeros trimmed) */
static void shortest(float v, uint64_t* ip, uint64_t* fp, int* dp) {
    const float av = fabsf(v);
    const double x = (double)av;
    const double hi = (x + (double)nextafterf(av, INFINITY)) * 0.5, lo = (x + (double)nextafterf(av, 0.0f)) * 0.5;
    int d = 0, low = 0, high = 0;
    double y = 0, fl = 0;
    for (;; ++d) {
        y = x * P10[d];
        fl = floor(y);
        low = fl > lo * P10[d];
        high = fl + 1.0 < hi * P10[d];
        if (low || high || d == 8) break;
    }
    int up;
    if (low == high) {                       /* both candidates identify x, or the 8-digit cut: nearest, ties to even */
        const double a = y - fl;
        up = a > 0.5 || (a == 0.5 && (((uint64_t)fl) & 1ull));
    } else {
        up = high;
    }
    uint64_t r = (uint64_t)fl + (uint64_t)up;
    while (d > 0 && r % 10 == 0) { r /= 10; --d; }
    *ip = r / I10[d];
    *fp = r % I10[d];
    *dp = d;
}

/* str(row) of numpy for a float32 row of n <= 64 elements; returns the length written (no terminator) or -1 */
int mcd_fmt_f32_row(const float* row, int n, char* out, int cap) {
    uint64_t ip[64], fp[64];
    int d[64], neg[64];
    if (n < 1 || n > 64) return -1;
    double amin = INFINITY, amax = 0.0;
    for (int i = 0; i < n; ++i) {
        const double a = fabs((double)row[i]);
        if (!(a >= 1.001e-4 && a < 16777216.0)) return -1;   /* also rejects NaN */
        if (a < amin) amin = a;
        if (a > amax) amax = a;
    }
    if (amax / amin > 999.0) return -1;
    int pl = 0, pr = 0;
    for (int i = 0; i < n; ++i) {
        shortest(row[i], &ip[i], &fp[i], &d[i]);
        neg[i] = row[i] < 0;
        const int li = ndigits(ip[i]) + neg[i];
        if (li > pl) pl = li;
        if (d[i] > pr) pr = d[i];
    }
    const int wlen = pl + 1 + pr;
    if (cap < 4 + n * (wlen + 2)) return -1;
    /* numpy _formatArray/_extendLine: lines start with one space, wrap before a word that would pass column 74 */
    char* o = out;
    int linelen = 1;          /* the leading space; replaced by '[' on the first line */
    *o++ = '[';
    for (int i = 0; i < n; ++i) {
        if (linelen + wlen > 74 && linelen > 1) {
            while (o > out && o[-1] == ' ') --o;   /* rstrip */
            *o++ = '\n';
            *o++ = ' ';
            linelen = 1;
        }
        char w[96];
        int k = wlen;
        /* fraction, right padded with spaces */
        for (int j = 0; j < pr - d[i]; ++j) w[--k] = ' ';
        uint64_t f = fp[i];
        for (int j = 0; j < d[i]; ++j) { w[--k] = (char)('0' + f % 10); f /= 10; }
        w[--k] = '.';
        uint64_t v = ip[i];
        do { w[--k] = (char)('0' + v % 10); v /= 10; } while (v);
        if (neg[i]) w[--k] = '-';
        while (k > 0) w[--k] = ' ';
        memcpy(o, w, (size_t)wlen);
        o += wlen;
        linelen += wlen;
        if (i + 1 < n) { *o++ = ' '; ++linelen; }
    }
    *o++ = ']';
    return (int)(o - out);
}

/* all rows of a [rows, n] matrix; lens[r] = length or -1; out has stride `cap` bytes per row */
void mcd_fmt_f32_rows(const float* a, int64_t rows, int n, char* out, int cap, int32_t* lens) {
    for (int64_t r = 0; r < rows; ++r) lens[r] = mcd_fmt_f32_row(a + r * n, n, out + r * cap, cap);
}

/* str(row) of numpy for an int64 row (describe_*_neurons.py: the `images` column, 5 image indices): every element
 * right-justified to the widest, one space between, no wrapping when the row fits 74 columns (else -1: numpy does it) */
int mcd_fmt_i64_row(const int64_t* row, int n, char* out, int cap) {
    if (n < 1 || n > 64) return -1;
    int w = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t v = row[i];
        if (v == INT64_MIN) return -1;
        const int l = ndigits((uint64_t)(v < 0 ? -v : v)) + (v < 0);
        if (l > w) w = l;
    }
    if ((w + 1) * n + 1 > 74 || cap < (w + 1) * n + 2) return -1;
    char* o = out;
    *o++ = '[';
    for (int i = 0; i < n; ++i) {
        char t[24];
        int k = w;
        const int64_t v = row[i];
        uint64_t a = (uint64_t)(v < 0 ? -v : v);
        do { t[--k] = (char)('0' + a % 10); a /= 10; } while (a);
        if (v < 0) t[--k] = '-';
        while (k > 0) t[--k] = ' ';
        memcpy(o, t, (size_t)w);
        o += w;
        if (i + 1 < n) *o++ = ' ';
    }
    *o++ = ']';
    return (int)(o - out);
}

void mcd_fmt_i64_rows(const int64_t* a, int64_t rows, int n, char* out, int cap, int32_t* lens) {
    for (int64_t r = 0; r < rows; ++r) lens[r] = mcd_fmt_i64_row(a + r * n, n, out + r * cap, cap);
}

/* ---- whole CSV rows of the og/broad drivers -------------------------------------------------------------------
 * layer,unit,description,similarity,images with Python's csv QUOTE_MINIMAL dialect (what pandas' to_csv drives): a
 * field is wrapped in '"' (inner '"' doubled) when it contains ',', '"', '\n' or '\r'.
 *   description = "[" + ", ".join(repr(word)) + "]"   (str() of the list of k concept strings; reprs come from Python)
 *   similarity  = str(np.float32[k])                  (mcd_fmt_f32_row)
 *   images      = str(np.int64[k_img])                (mcd_fmt_i64_row)
 * Returns the bytes written, or -1 when a row needs numpy's own formatting or `cap` is too small (the caller then
 * takes the csv-module path for the file). */
static char* emit_field(char* o, const char* t, int64_t n) {
    int special = 0;
    for (int64_t i = 0; i < n; ++i) {
        const char ch = t[i];
        if (ch == ',' || ch == '"' || ch == '\n' || ch == '\r') { special = 1; break; }
    }
    if (!special) { memcpy(o, t, (size_t)n); return o + n; }
    *o++ = '"';
    for (int64_t i = 0; i < n; ++i) {
        if (t[i] == '"') *o++ = '"';
        *o++ = t[i];
    }
    *o++ = '"';
    return o;
}

int64_t mcd_csv_og_rows(const char* layer, int layer_len, int64_t nrows, const int32_t* ids, int k,
                        const char* const* reprs, const int32_t* repr_lens, int n_words, const float* vals,
                        const int64_t* imgs, int k_img, char* out, int64_t cap) {
    char* o = out;
    char cell[4096];
    int64_t max_desc = 2;
    for (int j = 0; j < n_words; ++j)
        if (repr_lens[j] + 2 > max_desc) max_desc = repr_lens[j] + 2;
    max_desc = max_desc * k + 2;                       /* "[" + k * (repr + ", ") + "]" */
    if (k < 1 || k > 64 || k_img < 1 || k_img > 64) return -1;
    for (int64_t r = 0; r < nrows; ++r) {
        if ((o - out) + 2 * (layer_len + max_desc) + 3 * 4096 + 64 > cap) return -1;
        o = emit_field(o, layer, layer_len);
        *o++ = ',';
        {   /* unit */
            char t[24];
            int n = 0;
            int64_t v = r;
            do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
            while (n) *o++ = t[--n];
        }
        *o++ = ',';
        {   /* description: built after its own start position, then quoted in place if needed */
            char* d = o + max_desc + 8;                 /* scratch beyond the widest possible quoted field */
            char* e = d;
            *e++ = '[';
            for (int j = 0; j < k; ++j) {
                const int32_t w = ids[r * k + j];
                if (w < 0 || w >= n_words) return -1;
                if (j) { *e++ = ','; *e++ = ' '; }
                memcpy(e, reprs[w], (size_t)repr_lens[w]);
                e += repr_lens[w];
            }
            *e++ = ']';
            o = emit_field(o, d, e - d);
        }
        *o++ = ',';
        int n = mcd_fmt_f32_row(vals + r * k, k, cell, (int)sizeof(cell));
        if (n < 0) return -1;
        o = emit_field(o, cell, n);
        *o++ = ',';
        n = mcd_fmt_i64_row(imgs + r * k_img, k_img, cell, (int)sizeof(cell));
        if (n < 0) return -1;
        o = emit_field(o, cell, n);
        *o++ = '\n';
    }
    return (int64_t)(o - out);
}

/* ---- the activation-cache container (include/mcd_cache.h, host half) ------------------------------------------
 * A cache file is torch.save's zip archive of ONE float32 tensor [n_rows, width]: the tensor's bytes are the stored
 * (uncompressed) record <name>/data/0.  The Python side writes the archive once with placeholder data
 * (concept_vit/utils.py) and hands over the byte offset of the record's data and of the two places where the zip
 * format keeps its CRC-32.  Here the rows are written over the placeholder as they arrive, the CRC runs along, and
 * mcd_cachefile_close puts the CRC in place and renames <name>.part to <name>: a file under its final name is always
 * complete. */
static _Thread_local char g_cache_err[512];

const char* mcd_cachefile_last_error(void) { return g_cache_err; }

static int cache_fail(const char* what, const char* path, int err) {
    if (err)
        snprintf(g_cache_err, sizeof g_cache_err, "%s: %s: %s", what, path ? path : "", strerror(err));
    else
        snprintf(g_cache_err, sizeof g_cache_err, "%s: %s", what, path ? path : "");
    return -1;
}

/* CRC-32 of zip / zlib (IEEE 802.3, reflected polynomial 0xEDB88320), slicing by 8.  mcd_zip_crc32(0, NULL, 0) == 0;
 * feeding the pieces of a buffer in order gives the CRC of the whole, as zlib.crc32(piece, crc) does. */
static uint32_t g_crc_tab[8][256];
static int g_crc_ready;

static void crc_init(void) {
    /* idempotent: threads that race here write the same values; the flag is set last */
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        g_crc_tab[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
        for (int t = 1; t < 8; ++t) g_crc_tab[t][i] = (g_crc_tab[t - 1][i] >> 8) ^ g_crc_tab[0][g_crc_tab[t - 1][i] & 0xffu];
    __atomic_store_n(&g_crc_ready, 1, __ATOMIC_RELEASE);
}

uint32_t mcd_zip_crc32(uint32_t crc, const void* buf, size_t n) {
    const unsigned char* p = (const unsigned char*)buf;
    if (!__atomic_load_n(&g_crc_ready, __ATOMIC_ACQUIRE)) crc_init();
    uint32_t c = ~crc;
    while (n && ((uintptr_t)p & 7u)) { c = g_crc_tab[0][(c ^ *p++) & 0xffu] ^ (c >> 8); --n; }
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;                     /* little-endian hosts only (x86-64, aarch64): the zip fields below assume it too */
        c = g_crc_tab[7][lo & 0xffu] ^ g_crc_tab[6][(lo >> 8) & 0xffu] ^ g_crc_tab[5][(lo >> 16) & 0xffu] ^ g_crc_tab[4][lo >> 24] ^
            g_crc_tab[3][hi & 0xffu] ^ g_crc_tab[2][(hi >> 8) & 0xffu] ^ g_crc_tab[1][(hi >> 16) & 0xffu] ^ g_crc_tab[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = g_crc_tab[0][(c ^ *p++) & 0xffu] ^ (c >> 8);
    return ~c;
}

typedef struct {
    int fd;
    int64_t n_rows, width, rows_done, data_off, crc_off[2];
    uint32_t crc;
    char *part, *final;
} mcd_cachefile;

static int write_all(int fd, const void* buf, size_t n, int64_t off) {
    const char* p = (const char*)buf;
    while (n) {
        const ssize_t w = pwrite(fd, p, n, (off_t)off);
        if (w < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        p += w;
        off += w;
        n -= (size_t)w;
    }
    return 0;
}

static void cachefile_drop(mcd_cachefile* f, int unlink_part) {
    if (f->fd >= 0) close(f->fd);
    if (unlink_part && f->part) unlink(f->part);
    free(f->part);
    free(f->final);
    free(f);
}

/* Opens the placeholder archive `part_path` (it must exist and reach past the data record) for writing in place.
 * crc_off_a / crc_off_b: byte offsets of the record's CRC-32 fields (central-directory entry; local header or, where the
 * writer used one, the data descriptor behind the data); pass the same offset twice if the archive has one. */
int mcd_cachefile_open(const char* part_path, const char* final_path, int64_t n_rows, int64_t width, int64_t data_off,
                       int64_t crc_off_a, int64_t crc_off_b, void** out) {
    if (!part_path || !final_path || !out) return cache_fail("mcd_cachefile_open", "NULL argument", 0);
    *out = NULL;
    if (n_rows < 0 || width <= 0 || data_off < 0 || crc_off_a < 0 || crc_off_b < 0 || n_rows > (INT64_MAX >> 3) / width)
        return cache_fail("mcd_cachefile_open: bad shape or offset", part_path, 0);
    const int64_t bytes = n_rows * width * 4, end = data_off + bytes;
    const int64_t c[2] = {crc_off_a, crc_off_b};
    for (int i = 0; i < 2; ++i)
        if (c[i] + 4 > data_off && c[i] < end)
            return cache_fail("mcd_cachefile_open: a CRC field lies inside the data record", part_path, 0);
    mcd_cachefile* f = (mcd_cachefile*)calloc(1, sizeof *f);
    if (!f) return cache_fail("mcd_cachefile_open: out of memory", part_path, 0);
    f->fd = -1;
    f->part = strdup(part_path);
    f->final = strdup(final_path);
    if (!f->part || !f->final) {
        cachefile_drop(f, 0);
        return cache_fail("mcd_cachefile_open: out of memory", part_path, 0);
    }
    f->fd = open(part_path, O_WRONLY | O_CLOEXEC);
    if (f->fd < 0) {
        const int e = errno;
        cachefile_drop(f, 0);
        return cache_fail("mcd_cachefile_open", part_path, e);
    }
    const off_t size = lseek(f->fd, 0, SEEK_END);
    if (size < 0 || (int64_t)size < end || (int64_t)size < crc_off_a + 4 || (int64_t)size < crc_off_b + 4) {
        cachefile_drop(f, 1);
        return cache_fail("mcd_cachefile_open: the placeholder archive is shorter than its record", part_path, 0);
    }
    f->n_rows = n_rows;
    f->width = width;
    f->data_off = data_off;
    f->crc_off[0] = crc_off_a;
    f->crc_off[1] = crc_off_b;
    *out = f;
    return 0;
}

/* rows row0 .. row0 + n - 1; the pieces must arrive in order (row0 == the rows written so far) */
int mcd_cachefile_append(void* h, const float* rows, int64_t row0, int64_t n) {
    mcd_cachefile* f = (mcd_cachefile*)h;
    if (!f || n < 0 || (n > 0 && !rows)) return cache_fail("mcd_cachefile_append", "bad argument", 0);
    if (row0 != f->rows_done) return cache_fail("mcd_cachefile_append: rows out of order", f->part, 0);
    if (n > f->n_rows - f->rows_done) return cache_fail("mcd_cachefile_append: more rows than the file was opened for", f->part, 0);
    const size_t bytes = (size_t)n * (size_t)f->width * 4;
    if (write_all(f->fd, rows, bytes, f->data_off + f->rows_done * f->width * 4) != 0) return cache_fail("mcd_cachefile_append", f->part, errno);
    f->crc = mcd_zip_crc32(f->crc, rows, bytes);
    f->rows_done += n;
    return 0;
}

/* Removes the .part file; nothing appears under the final name. */
void mcd_cachefile_abort(void* h) {
    if (h) cachefile_drop((mcd_cachefile*)h, 1);
}

/* Finalises: CRC fields, close, rename to the final name.  With rows missing it is an error and acts as abort.  The handle is
 * gone either way. */
int mcd_cachefile_close(void* h) {
    mcd_cachefile* f = (mcd_cachefile*)h;
    if (!f) return cache_fail("mcd_cachefile_close", "NULL handle", 0);
    int rc = 0;
    if (f->rows_done != f->n_rows) {
        snprintf(g_cache_err, sizeof g_cache_err, "mcd_cachefile_close: %s holds %lld of %lld rows", f->part,
                 (long long)f->rows_done, (long long)f->n_rows);
        rc = -1;
    }
    unsigned char le[4] = {(unsigned char)f->crc, (unsigned char)(f->crc >> 8), (unsigned char)(f->crc >> 16), (unsigned char)(f->crc >> 24)};
    for (int i = 0; i < 2 && rc == 0; ++i)
        if (write_all(f->fd, le, 4, f->crc_off[i]) != 0) rc = cache_fail("mcd_cachefile_close", f->part, errno);
    if (rc == 0) {
        const int fd = f->fd;
        f->fd = -1;
        if (close(fd) != 0) rc = cache_fail("mcd_cachefile_close", f->part, errno);
    }
    if (rc == 0 && rename(f->part, f->final) != 0) rc = cache_fail("mcd_cachefile_close: rename", f->final, errno);
    cachefile_drop(f, rc != 0);
    return rc;
}
