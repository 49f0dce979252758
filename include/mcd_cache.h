/*
 * mcd_cache.h -- streaming the reference-format activation-cache files out while the encoder runs.
 *
 * Three parts, two libraries:
 *   1. libmcd_hip.so   mcd_hook_pool_rows: K0 (mcd_hook_pool) that also stores the pooled block row-major, the layout of
 *                      the layer's cache file [N, U_layer];
 *   2. libmcd_hip.so   mcd_cache_stream_*: one copy stream, a ring of pinned host slots and one worker thread that take
 *                      such blocks off the device and hand them to the container;
 *   3. libmcd_host.so  mcd_cachefile_* / mcd_zip_crc32: the container, plain C without a GPU (csrc/mcd_host.c).
 * libmcd_hip.so does not link libmcd_host.so: mcd_cache_stream_open takes the container's entry points as a table of
 * function pointers (mcd_cache_io_t), so either library loads without the other.
 * Same conventions as include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes, with the
 * exceptions written at each entry.  Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are
 * _lib.CACHE_SIGNATURES (libmcd_hip.so) and _lib.CACHE_HOST_SIGNATURES (libmcd_host.so).
 */
#ifndef MCD_CACHE_H
#define MCD_CACHE_H

#include <stddef.h>
#include <stdint.h>

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K0 with two stores.  Everything mcd_hook_pool does with (x, B, Cout, HW, mode, dst, row0, col0, stride_n, stride_u),
 * from the same loads and the same arithmetic, so dst receives the same bits; in addition
 *          rows[b*width + f] = the value stored for image b, neuron f            b < B, f < Cout,
 * a [B, width] row-major block with width >= Cout (floats f >= Cout of a row are not written).  rows must not overlap
 * the written part of dst.  Asynchronous on `stream`, hipGraph-capturable, one launch, no workspace.
 * MCD_E_ARG: what mcd_hook_pool rejects, rows == NULL, width < Cout.
 * ------------------------------------------------------------------------------------------- */
int mcd_hook_pool_rows(const float* x, int64_t B, int64_t Cout, int64_t HW, int mode, float* dst, int64_t row0,
                       int64_t col0, int64_t stride_n, int64_t stride_u, float* rows, int64_t width,
                       mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The container's entry points as mcd_cache_stream_open takes them (the mcd_cachefile_* functions below, or stand-ins
 * of the same contract).  Called on the worker thread only, except abort, which close may call on the closing thread
 * after the worker has ended.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int (*append)(void* file, const float* rows, int64_t row0, int64_t n);
    int (*close)(void* file);
    void (*abort)(void* file);
    const char* (*last_error)(void);
} mcd_cache_io_t;

/* ---------------------------------------------------------------------------------------------
 * The stream writer.  NOT hipGraph-capturable and not free of host effects, unlike the kernels: open allocates (the ring
 * of pinned slots once per process, reused by every later writer that fits it) and starts the worker thread; push may
 * block on the host while every slot is still owned by the worker; close joins the worker.  None of them synchronises
 * the device or touches the NULL stream: the copies run on a non-blocking stream of the writer's own.
 *
 * open    n_files files, files[i] an open container handle (mcd_cachefile_open) of widths[i] floats per row, which the
 *         writer owns from here on.  n_slots >= 1 slots of slot_bytes each; a push moves at most slot_bytes.  The
 *         device is the calling thread's current one.  On an error the files are aborted.
 * reserve makes `stream` wait until the writer has finished READING the device block given to the last push of `file`
 *         (a hipStreamWaitEvent: nothing blocks on the host).  Call it before the kernel that overwrites a staging
 *         block that an earlier push of that file read.
 * push    rows row0 .. row0 + n - 1 of `file` lie at device_block, [n, widths[file]] row-major, written by work queued
 *         on `stream` before this call.  Records an event on `stream`, makes the copy stream wait for it, queues the
 *         device -> pinned-host copy into a free slot (waits on the host for one if none is free), records the
 *         slot's done-event and posts the job.  The worker waits for that event and appends the rows to the file.
 *         Pushes of one file must come in row order.  n == 0 is MCD_OK and does nothing.
 * close   waits until every posted job is written, finalises every file (CRC fields, rename from .part), joins the
 *         worker, frees the handle and returns MCD_OK, or the FIRST error any push, copy, append or finalisation
 *         met -- with its text in mcd_last_error() -- after removing every file that was not finalised.  It never aborts
 *         the process.
 * abort   as close, but finalises nothing: every .part file is removed.
 * MCD_E_ARG: NULL / out-of-range arguments, n * widths[file] * 4 > slot_bytes.  MCD_E_LAUNCH: a HIP call failed.
 * MCD_E_UNSUPPORTED (from close): a container call failed.
 * ------------------------------------------------------------------------------------------- */
int mcd_cache_stream_open(int n_files, void* const* files, const int64_t* widths, const mcd_cache_io_t* io, int n_slots,
                          size_t slot_bytes, void** handle);
int mcd_cache_stream_reserve(void* handle, int file, mcd_stream_t stream);
int mcd_cache_stream_push(void* handle, int file, const float* device_block, int64_t row0, int64_t n,
                          mcd_stream_t stream);
int mcd_cache_stream_close(void* handle);
int mcd_cache_stream_abort(void* handle);

/* ---------------------------------------------------------------------------------------------
 * The container (libmcd_host.so; errors return -1 with the text in mcd_cachefile_last_error(), thread-local).
 * A cache file is torch.save's zip archive of one float32 tensor [n_rows, width], whose bytes are one stored record.
 * The archive is written first with placeholder data as <name>.part; these entries write the rows over the placeholder,
 * keep the record's CRC-32 and, on close, put it into the archive's two CRC fields and rename the file to <name>.
 *
 * mcd_zip_crc32      zlib.crc32(buf[:n], crc): the IEEE polynomial, table driven; (0, NULL, 0) -> 0.
 * mcd_cachefile_open part_path exists and holds the archive; data_off the first byte of the record's data; crc_off_a,
 *                    crc_off_b the byte offsets of its CRC-32 fields (the central-directory entry's, and the local
 *                    header's or -- where the archive's writer used one -- the data descriptor's behind the data).
 * mcd_cachefile_append  rows row0 .. row0 + n - 1; row0 must equal the rows appended so far and the total must not
 *                    pass n_rows, else -1 and nothing is written.
 * mcd_cachefile_close   with all n_rows rows in: CRC fields, close, rename; else -1 and the .part file is removed.
 *                    The handle is gone either way.
 * mcd_cachefile_abort   removes the .part file and the handle.
 * ------------------------------------------------------------------------------------------- */
uint32_t mcd_zip_crc32(uint32_t crc, const void* buf, size_t n);
int mcd_cachefile_open(const char* part_path, const char* final_path, int64_t n_rows, int64_t width, int64_t data_off,
                       int64_t crc_off_a, int64_t crc_off_b, void** out);
int mcd_cachefile_append(void* file, const float* rows, int64_t row0, int64_t n);
int mcd_cachefile_close(void* file);
void mcd_cachefile_abort(void* file);
const char* mcd_cachefile_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MCD_CACHE_H */
