/* cache_host_check.c -- a stand-alone driver of the container entries of include/mcd_cache.h (csrc/mcd_host.c), meant to be
 * compiled TOGETHER with mcd_host.c under -fsanitize=address,undefined and run directly (tests/test_cache_stream_cpu.py does):
 *     cache_host_check <directory>
 * It needs no torch: the "archive" is a hand-made file with the three regions the container knows about -- some header bytes,
 * the data record, a trailer with the two CRC fields -- and the checks are on the bytes of the finished file.
 * Exit status 0 and "cache_host_check: OK" when every check holds. */
#define _POSIX_C_SOURCE 200809L   /* access, unlink */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "mcd_cache.h"

static int failures;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

/* the bitwise definition of the zip CRC-32, to hold the table-driven one against */
static uint32_t crc_bitwise(uint32_t crc, const unsigned char* p, size_t n) {
    crc = ~crc;
    while (n--) {
        crc ^= *p++;
        for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
    }
    return ~crc;
}

static int exists(const char* path) { return access(path, F_OK) == 0; }

enum { HEAD = 37, TRAIL = 24 };   /* odd sizes on purpose: nothing is aligned */

static void make_placeholder(const char* part, int64_t n, int64_t u) {
    FILE* f = fopen(part, "wb");
    if (!f) { perror(part); exit(2); }
    const size_t total = HEAD + (size_t)(n * u * 4) + TRAIL;
    unsigned char* b = (unsigned char*)malloc(total);
    memset(b, 0xAB, total);
    fwrite(b, 1, total, f);
    free(b);
    fclose(f);
}

static unsigned char* slurp(const char* path, size_t* size) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* b = (unsigned char*)malloc(*size ? *size : 1);
    if (fread(b, 1, *size, f) != *size) { free(b); b = NULL; }
    fclose(f);
    return b;
}

static void one_file(const char* dir, int64_t n, int64_t u, const int64_t* pieces, int n_pieces) {
    char part[4096], fin[4096];
    snprintf(fin, sizeof fin, "%s/check_%lld_%lld.pt", dir, (long long)n, (long long)u);
    snprintf(part, sizeof part, "%s.part", fin);
    const size_t count = (size_t)(n * u);
    uint32_t* src = (uint32_t*)malloc(count * 4 + 4);
    uint32_t x = 0x9E3779B9u ^ (uint32_t)(n * 131 + u);
    for (size_t i = 0; i < count; ++i) { x = x * 1664525u + 1013904223u; src[i] = x; }
    const uint32_t special[] = {0x7fc00000u, 0xffc00001u, 0x7f800000u, 0xff800000u, 0x80000000u};
    for (size_t i = 0; i < count && i < 5; ++i) src[i] = special[i];

    make_placeholder(part, n, u);
    const int64_t data_off = HEAD, crc_a = HEAD + n * u * 4 + 3, crc_b = HEAD + n * u * 4 + 17;
    void* h = NULL;
    CHECK(mcd_cachefile_open(part, fin, n, u, data_off, crc_a, crc_b, &h) == 0 && h);
    if (!h) { free(src); return; }
    int64_t row0 = 0;
    for (int i = 0; i < n_pieces; ++i) {
        /* each piece from an exactly sized heap block: a read past its end is the sanitizer's to catch */
        const size_t bytes = (size_t)(pieces[i] * u * 4);
        float* piece = (float*)malloc(bytes ? bytes : 1);
        memcpy(piece, src + row0 * u, bytes);
        CHECK(mcd_cachefile_append(h, piece, row0, pieces[i]) == 0);
        free(piece);
        row0 += pieces[i];
        CHECK(!exists(fin));
    }
    CHECK(row0 == n);
    CHECK(mcd_cachefile_append(h, (const float*)src, row0, 1) != 0);        /* past the last row */
    CHECK(strstr(mcd_cachefile_last_error(), "more rows") != NULL);
    CHECK(mcd_cachefile_close(h) == 0);
    CHECK(exists(fin) && !exists(part));

    size_t size = 0;
    unsigned char* b = slurp(fin, &size);
    CHECK(b && size == HEAD + count * 4 + TRAIL);
    if (b && size == HEAD + count * 4 + TRAIL) {
        const uint32_t want = crc_bitwise(0, (const unsigned char*)src, count * 4);
        CHECK(memcmp(b + HEAD, src, count * 4) == 0);
        uint32_t a, c;
        memcpy(&a, b + crc_a, 4);
        memcpy(&c, b + crc_b, 4);
        CHECK(a == want && c == want);
        for (size_t i = 0; i < HEAD; ++i) CHECK(b[i] == 0xAB);
        for (size_t i = HEAD + count * 4; i < size; ++i)
            CHECK(b[i] == 0xAB || (i >= (size_t)crc_a && i < (size_t)crc_a + 4) || (i >= (size_t)crc_b && i < (size_t)crc_b + 4));
    }
    free(b);
    free(src);
    unlink(fin);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
    const char* dir = argv[1];

    /* the CRC against its bitwise definition: empty, every split of 9 bytes, every start alignment */
    CHECK(mcd_zip_crc32(0, NULL, 0) == 0);
    const unsigned char nine[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    CHECK(mcd_zip_crc32(0, nine, 9) == 0xCBF43926u);
    for (size_t cut = 0; cut <= 9; ++cut) CHECK(mcd_zip_crc32(mcd_zip_crc32(0, nine, cut), nine + cut, 9 - cut) == 0xCBF43926u);
    for (size_t len = 0; len < 70; ++len) {
        unsigned char* buf = (unsigned char*)malloc(len + 8);
        for (size_t i = 0; i < len + 8; ++i) buf[i] = (unsigned char)(i * 37 + len);
        for (size_t off = 0; off < 8; ++off) CHECK(mcd_zip_crc32(5, buf + off, len) == crc_bitwise(5, buf + off, len));
        free(buf);
    }

    const int64_t p1[] = {2, 3}, p2[] = {100, 100, 57}, p3[] = {1}, p4[] = {0, 4, 0};
    one_file(dir, 5, 3, p1, 2);
    one_file(dir, 257, 768, p2, 3);
    one_file(dir, 1, 1, p3, 1);
    one_file(dir, 4, 2, p4, 3);

    /* a close before all rows arrived, out-of-order rows, an abort: nothing is left under either name */
    char part[4096], fin[4096];
    snprintf(fin, sizeof fin, "%s/check_short.pt", dir);
    snprintf(part, sizeof part, "%s.part", fin);
    float rows[6] = {1, 2, 3, 4, 5, 6};
    void* h = NULL;
    make_placeholder(part, 5, 3);
    CHECK(mcd_cachefile_open(part, fin, 5, 3, HEAD, HEAD + 60, HEAD + 64, &h) == 0);
    CHECK(mcd_cachefile_append(h, rows, 1, 2) != 0);
    CHECK(mcd_cachefile_append(h, rows, 0, 2) == 0);
    CHECK(mcd_cachefile_append(h, rows, 0, 2) != 0);
    CHECK(mcd_cachefile_close(h) != 0);
    CHECK(strstr(mcd_cachefile_last_error(), "2 of 5 rows") != NULL);
    CHECK(!exists(fin) && !exists(part));
    make_placeholder(part, 5, 3);
    CHECK(mcd_cachefile_open(part, fin, 5, 3, HEAD, HEAD + 60, HEAD + 64, &h) == 0);
    mcd_cachefile_abort(h);
    CHECK(!exists(fin) && !exists(part));
    /* refused opens: a record longer than the file, a CRC field inside the data, no such file, bad shapes */
    make_placeholder(part, 5, 3);
    CHECK(mcd_cachefile_open(part, fin, 5, 3, HEAD, HEAD + 10, HEAD + 64, &h) != 0 && h == NULL);
    CHECK(mcd_cachefile_open(part, fin, 5, 0, HEAD, HEAD + 60, HEAD + 64, &h) != 0);
    CHECK(mcd_cachefile_open(part, fin, -1, 3, HEAD, HEAD + 60, HEAD + 64, &h) != 0);
    CHECK(mcd_cachefile_open(part, fin, INT64_MAX / 2, 3, HEAD, HEAD + 60, HEAD + 64, &h) != 0);
    CHECK(mcd_cachefile_open(NULL, fin, 5, 3, HEAD, HEAD + 60, HEAD + 64, &h) != 0);
    CHECK(exists(part));
    CHECK(mcd_cachefile_open(part, fin, 50, 3, HEAD, HEAD + 600, HEAD + 604, &h) != 0);      /* removes the short placeholder */
    CHECK(!exists(part));
    CHECK(mcd_cachefile_open(part, fin, 5, 3, HEAD, HEAD + 60, HEAD + 64, &h) != 0);
    CHECK(mcd_cachefile_close(NULL) != 0);
    mcd_cachefile_abort(NULL);

    if (failures) {
        fprintf(stderr, "cache_host_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    printf("cache_host_check: OK\n");
    return 0;
}
