/*
 * h5_direct.c -- direct-chunk HDF5 file <-> VRAM path (include/deltarice_h5io.h).
 * Host-side caller of the hot path: HDF5 chunk I/O + one PCIe copy + one batched drx_* call.
 *
 * The entry points are made of: dataset_t, the SOURCE (open_dataset, source_plan, same_file); fetched_t, stored chunks on the
 * device (fetch_rows_chunks; fill_by_pread / fill_by_read_chunk for drx_h5_read's pipelined fetch of all of them); padded_t, the
 * last chunk of a dataset whose rows do not fill it (pad_*); result_t, new chunks on the device and on the host (result_to_host);
 * dst_t, the DESTINATION file (dst_create, dst_write_chunks, dst_close; dst_store: all three).  A call owns one call_t of
 * these and releases it with call_release().  What is computed from numbers alone is h5_direct_plan.h.
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <dlfcn.h>
#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <hdf5.h>
#include <pthread.h>
#include <stdio.h>
#include <unistd.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <string.h>
#include <time.h>

#include "deltarice_h5io.h"
#include "h5_direct_plan.h"

#define FILTER_ID 32025

static double now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* H5Dcreate refuses a MANDATORY filter it cannot find, although H5Dwrite_chunk never runs it: make
 * filter 32025 known to this process' HDF5 by registering the plugin that sits next to this library. */
static void ensure_filter_registered(void) {
    static int done;
    if (done || H5Zfilter_avail(FILTER_ID) > 0) { done = 1; return; }
    Dl_info info;
    if (dladdr((void *)&ensure_filter_registered, &info) && info.dli_fname) {
        char path[4096];
        snprintf(path, sizeof path, "%s", info.dli_fname);
        char *slash = strrchr(path, '/');
        if (slash) {
            snprintf(slash + 1, sizeof path - (size_t)(slash + 1 - path), "plugin/libh5deltarice.so");
            void *h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
            if (h) {
                /* register through THIS library's libhdf5 (the plugin itself does not link one) */
                const void *(*info_fn)(void) = (const void *(*)(void))dlsym(h, "H5PLget_plugin_info");
                if (info_fn) (void)H5Zregister(info_fn());
            }
        }
    }
    done = 1;
}

/* The raw hipMalloc / hipMemcpy calls below must land on the context's device whatever device the calling thread has
 * current (include/deltarice_hip.h: every call runs on the context's device and restores the caller's). */
static int enter_device(const drx_ctx *ctx, int *prev) {
    const int want = drx_ctx_device(ctx);
    if (hipGetDevice(prev) != hipSuccess) *prev = -1;
    if (*prev == want) { *prev = -1; return 0; }  /* nothing to restore */
    return hipSetDevice(want) == hipSuccess ? 0 : -1;
}

/* A second stream for the copies of this path (one per device, made on first use, never destroyed): chunk data crosses
 * PCIe on it while the calling thread is inside HDF5. */
static hipStream_t copy_stream_of(int dev) {
    static hipStream_t cs[64];
    if (dev < 0 || dev >= 64) return NULL;
    if (!cs[dev] && hipStreamCreateWithFlags(&cs[dev], hipStreamNonBlocking) != hipSuccess) cs[dev] = NULL;
    return cs[dev];
}

static int log2_m(unsigned m, unsigned *k) {
    if (m == 0 || (m & (m - 1)) || m > 32768) return -1;
    *k = 0;
    while ((1u << *k) != m) ++*k;
    return 0;
}

/* ---- the source ---- */

/* A dataset this path takes (include/deltarice_h5io.h), opened read-only: its extent, chunk shape, a copy of its element type,
 * its cd_values as stored and parsed.  Returns DRX_OK with all handles open, or the status to report with whatever was opened
 * left for close_dataset(). */
typedef struct {
    hid_t f, d, sp, pl, ty;
    hsize_t dims[2], chunk[2];
    drx_opts o;
    unsigned cd[3 + DRX_MAX_TAPS], flags;
    size_t ncd;
} dataset_t;
static void close_dataset(dataset_t *ds) {
    if (ds->ty >= 0) H5Tclose(ds->ty);
    if (ds->pl >= 0) H5Pclose(ds->pl);
    if (ds->sp >= 0) H5Sclose(ds->sp);
    if (ds->d >= 0) H5Dclose(ds->d);
    if (ds->f >= 0) H5Fclose(ds->f);
    ds->f = ds->d = ds->sp = ds->pl = ds->ty = -1;
}
static drx_status open_dataset(const char *file, const char *name, dataset_t *ds) {
    if ((ds->f = H5Fopen(file, H5F_ACC_RDONLY, H5P_DEFAULT)) < 0) return DRX_ERR_ARG;
    if ((ds->d = H5Dopen2(ds->f, name, H5P_DEFAULT)) < 0) return DRX_ERR_ARG;
    ds->sp = H5Dget_space(ds->d);
    ds->pl = H5Dget_create_plist(ds->d);
    if (H5Sget_simple_extent_ndims(ds->sp) != 2 || H5Sget_simple_extent_dims(ds->sp, ds->dims, NULL) < 0) return DRX_ERR_ARG;
    if (H5Pget_chunk(ds->pl, 2, ds->chunk) != 2 || ds->chunk[1] != ds->dims[1]) return DRX_ERR_UNSUPPORTED;
    {
        hid_t ty = H5Dget_type(ds->d);
        /* 16-bit integers in the byte order the codec computes in; signed or unsigned alike (the reference reinterprets the
         * bytes as int16 whatever the type, tests/test.py:72-83) */
        const int ok = H5Tget_class(ty) == H5T_INTEGER && H5Tget_size(ty) == 2 && H5Tget_order(ty) == H5T_ORDER_LE;
        ds->ty = H5Tcopy(ty);  /* (what a new dataset of another file is created with) */
        H5Tclose(ty);
        if (!ok) return DRX_ERR_UNSUPPORTED;
    }
    unsigned fcfg = 0;
    char fname[8];
    ds->ncd = 3 + DRX_MAX_TAPS;
    if (H5Pget_nfilters(ds->pl) != 1 ||
        H5Pget_filter_by_id2(ds->pl, FILTER_ID, &ds->flags, &ds->ncd, ds->cd, sizeof fname, fname, &fcfg) < 0)
        return DRX_ERR_UNSUPPORTED;  /* other filters in the pipeline */
    if (drx_parse_cd_values(ds->ncd, ds->cd, &ds->o) != DRX_OK) return DRX_ERR_ARG;
    return DRX_OK;
}

/* A uniform plan over n_chunks of the source's chunks with its RiceParameter, WaveformLength and filter. */
static drx_status source_plan(drx_ctx *ctx, const dataset_t *ds, uint64_t n_chunks, drx_plan **plan) {
    const drx_status rc = drx_plan_create_uniform(ctx, n_chunks, (uint32_t)(ds->chunk[0] * ds->chunk[1]),
                                                  ds->o.wave_len < 0 ? 0u : (uint32_t)ds->o.wave_len, ds->o.rice_k, plan);
    return rc != DRX_OK ? rc : drx_plan_set_filter(*plan, ds->o.n_taps, ds->o.taps);
}

/* The same file under either name, a hard link included (dst may not exist yet). */
static int same_file(const char *src, const char *dst) {
    struct stat a, b;
    return !strcmp(src, dst) || (stat(src, &a) == 0 && stat(dst, &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino);
}

/* ---- what a call owns ---- */

/* Stored chunks of the source on the device, and (fetch_rows_chunks) the rows as waveform indices of a uniform plan over them. */
typedef struct {
    uint64_t *touched, *h_off, *h_addr, *d_off, *wave_idx;  /* sorted chunk numbers; word offsets, file addresses; n_rows * wpr indices */
    void *d_words;
    uint64_t n_touched, words;  /* chunks fetched, their words */
} fetched_t;

/* The last chunk of a dataset whose rows do not fill it (HDF5 stores it full size, padded with the fill value 0): a sample buffer
 * of a whole chunk, a one-chunk plan, and for a new dataset (pad_open) a buffer of its own for the words.  pad_encode() launches,
 * pad_finish() waits and learns the words, so that a caller can do other work between the two. */
typedef struct { drx_plan *plan; void *d_samples, *d_words; uint64_t cap, words; } padded_t;

/* New chunks on the device (d_words, d_off) and their offsets on the host. */
typedef struct { void *d_words; uint64_t *d_off, *h_off; } result_t;

typedef struct {
    int prev_dev;
    drx_h5_stats s;
    dataset_t ds;
    fetched_t fx;
    drx_plan *plan;
    padded_t pad;
    result_t res;
    uint64_t *rows;
} call_t;
static int call_begin(call_t *c, drx_ctx *ctx) {
    memset(c, 0, sizeof *c);
    c->ds.f = c->ds.d = c->ds.sp = c->ds.pl = c->ds.ty = -1;
    return enter_device(ctx, &c->prev_dev);
}
/* Every entry point's last step.  Plans first: destroying one drains its work, then the buffers its kernels used are freed. */
static drx_status call_release(call_t *c, drx_h5_stats *st, drx_status rc) {
    drx_plan_destroy(c->plan);
    drx_plan_destroy(c->pad.plan);
    void *dev[] = {c->pad.d_samples, c->pad.d_words, c->res.d_words, c->res.d_off, c->fx.d_words, c->fx.d_off};
    void *host[] = {c->res.h_off, c->rows, c->fx.touched, c->fx.wave_idx, c->fx.h_off, c->fx.h_addr};
    for (size_t i = 0; i < sizeof dev / sizeof *dev; ++i) (void)hipFree(dev[i]);
    for (size_t i = 0; i < sizeof host / sizeof *host; ++i) free(host[i]);
    close_dataset(&c->ds);
    if (c->prev_dev >= 0) (void)hipSetDevice(c->prev_dev);
    if (st) *st = c->s;
    return rc;
}

/* ---- drx_h5_read: the whole dataset's stored chunks to the staging buffer and on to the device, slab by slab ---- */

static int slab_to_device(const slab_t *sl, const uint64_t *h_off, const void *h_words, void *d_words, hipStream_t stream) {
    const uint64_t w0 = h_off[sl->c0], w1 = h_off[sl->c1];
    return hipMemcpyAsync((uint32_t *)d_words + w0, (const uint32_t *)h_words + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, stream) == hipSuccess ? 0 : -1;
}

/* file -> pinned memory by plain pread(2) from several threads, where HDF5 tells where the chunks lie (H5Dget_chunk_info_by_coord,
 * 1.10.5+) and the file is one the operating system can read as it is (sec2 driver, no user block, opened read-only): four
 * threads copy out of the page cache at several times the rate of one, and H5Dread_chunk is one thread by construction. */
typedef struct {
    int fd;
    const uint64_t *addr, *off_words;  /* per chunk: file address, word offset in the staging buffer */
    uint8_t *dst;
    const slab_t *slabs;
    int n_slabs, n_threads, failed;
    int done[kMaxSlabs];
    pthread_mutex_t mu;
    pthread_cond_t cv;
} raw_reader;
typedef struct { raw_reader *r; int t; } raw_arg;
static void *raw_reader_main(void *p) {
    raw_arg *a = (raw_arg *)p;
    raw_reader *r = a->r;
    for (int s = a->t; s < r->n_slabs; s += r->n_threads) {
        int ok = 1;
        for (uint64_t c = r->slabs[s].c0; c < r->slabs[s].c1 && ok; ++c) {
            uint64_t left = (r->off_words[c + 1] - r->off_words[c]) * 4, at = 0;
            while (left) {
                const ssize_t got = pread(r->fd, r->dst + r->off_words[c] * 4 + at, left, (off_t)(r->addr[c] + at));
                if (got <= 0) { ok = 0; break; }
                left -= (uint64_t)got; at += (uint64_t)got;
            }
        }
        pthread_mutex_lock(&r->mu);
        r->done[s] = 1;
        if (!ok) r->failed = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
    }
    return NULL;
}
/* Up to four threads read the slabs from fd (closed here); the copy of slab s to the device is issued as soon as slab s is done. */
static drx_status fill_by_pread(int fd, const fetched_t *fx, void *h_words, const slab_t *slabs, int n_slabs, hipStream_t stream) {
    raw_reader rr;
    memset(&rr, 0, sizeof rr);
    rr.fd = fd; rr.addr = fx->h_addr; rr.off_words = fx->h_off; rr.dst = (uint8_t *)h_words; rr.slabs = slabs; rr.n_slabs = n_slabs;
    rr.n_threads = n_slabs < 4 ? n_slabs : 4;
    pthread_mutex_init(&rr.mu, NULL);
    pthread_cond_init(&rr.cv, NULL);
    pthread_t th[4];
    raw_arg args[4];
    int started = 0;
    for (int t = 0; t < rr.n_threads; ++t) {
        args[t].r = &rr; args[t].t = t;
        if (pthread_create(&th[t], NULL, raw_reader_main, &args[t]) != 0) break;
        ++started;
    }
    int bad = started != rr.n_threads;
    if (bad) {  /* (the slabs of a thread that did not start would never be done) */
        pthread_mutex_lock(&rr.mu);
        rr.failed = 1;
        pthread_mutex_unlock(&rr.mu);
    }
    for (int sl = 0; sl < n_slabs && !bad; ++sl) {
        pthread_mutex_lock(&rr.mu);
        while (!rr.done[sl] && !rr.failed) pthread_cond_wait(&rr.cv, &rr.mu);
        bad = rr.failed;
        pthread_mutex_unlock(&rr.mu);
        if (!bad && slab_to_device(&slabs[sl], fx->h_off, h_words, fx->d_words, stream) != 0) bad = 1;
    }
    for (int t = 0; t < started; ++t) pthread_join(th[t], NULL);
    pthread_mutex_destroy(&rr.mu);
    pthread_cond_destroy(&rr.cv);
    close(fd);
    if (bad) (void)hipStreamSynchronize(stream);
    return bad ? DRX_ERR_CORRUPT : DRX_OK;
}
/* Any other file: H5Dread_chunk, one thread, each slab on its way to the device while the next one is read. */
static drx_status fill_by_read_chunk(const dataset_t *ds, const fetched_t *fx, void *h_words, const slab_t *slabs, int n_slabs, hipStream_t stream) {
    for (int sl = 0; sl < n_slabs; ++sl) {
        for (uint64_t c = slabs[sl].c0; c < slabs[sl].c1; ++c) {
            hsize_t off[2] = {c * ds->chunk[0], 0};
            uint32_t mask = 0;
            if (H5Dread_chunk(ds->d, H5P_DEFAULT, off, &mask, (uint32_t *)h_words + fx->h_off[c]) < 0 || mask) {
                (void)hipStreamSynchronize(stream);
                return DRX_ERR_CORRUPT;
            }
        }
        if (slab_to_device(&slabs[sl], fx->h_off, h_words, fx->d_words, stream) != 0) return DRX_ERR_DEVICE;
    }
    return DRX_OK;
}

/* The stored sizes of the dataset's n_chunks chunks as word offsets h_off[n_chunks + 1] and, where HDF5 tells them, their file
 * addresses h_addr[n_chunks]; *raw_ok: the file is one plain preads can read (every chunk has an address and no filter was
 * skipped, sec2 driver, no user block, opened read-only, DRX_H5_NO_RAW not set, HDF5 1.10.5 or later). */
static drx_status chunk_table(const dataset_t *ds, uint64_t n_chunks, uint64_t *h_off, uint64_t *h_addr, int *raw_ok) {
    uint64_t words = 0;
    *raw_ok = 1;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        hsize_t off[2] = {c * ds->chunk[0], 0}, nb = 0;
#if H5_VERSION_GE(1, 10, 5)
        unsigned fmask = 0;
        haddr_t addr = HADDR_UNDEF;
        if (H5Dget_chunk_info_by_coord(ds->d, off, &fmask, &addr, &nb) < 0 || (nb & 3)) return DRX_ERR_CORRUPT;
        if (addr == HADDR_UNDEF || fmask) *raw_ok = 0;
        h_addr[c] = (uint64_t)addr;
        if (addr == HADDR_UNDEF) nb = 0;
#else
        *raw_ok = 0;
        h_addr[c] = 0;
        if (H5Dget_chunk_storage_size(ds->d, off, &nb) < 0 || (nb & 3)) return DRX_ERR_CORRUPT;
#endif
        if (nb == 0) return DRX_ERR_UNSUPPORTED;  /* a chunk that was never written (fill value): not a stored stream */
        h_off[c] = words;
        words += nb / 4;
    }
    h_off[n_chunks] = words;
    if (*raw_ok) {  /* a file the operating system can read as it is? */
        hid_t fapl = H5Fget_access_plist(ds->f), fcpl = H5Fget_create_plist(ds->f);
        hsize_t ub = 1;
        unsigned intent = H5F_ACC_RDWR;
        if (fapl < 0 || fcpl < 0 || H5Pget_driver(fapl) != H5FD_SEC2 || H5Pget_userblock(fcpl, &ub) < 0 || ub != 0 ||
            H5Fget_intent(ds->f, &intent) < 0 || intent != H5F_ACC_RDONLY || getenv("DRX_H5_NO_RAW"))
            *raw_ok = 0;
        if (fapl >= 0) H5Pclose(fapl);
        if (fcpl >= 0) H5Pclose(fcpl);
    }
    return DRX_OK;
}

drx_status drx_h5_read(drx_ctx *ctx, const char *file, const char *name, int16_t *d_out,
                       uint64_t out_cap_samples, drx_h5_stats *st) {
    if (!ctx || !file || !name || !d_out) return DRX_ERR_ARG;
    call_t c;
    double t0 = now();
    if (call_begin(&c, ctx) != 0) return DRX_ERR_DEVICE;
    drx_h5_stats *s = &c.s;
    fetched_t *fx = &c.fx;
    void *h_words = NULL;  /* (the context's staging buffer, not freed here) */
    hipStream_t stream = (hipStream_t)drx_ctx_stream(ctx);

    drx_status rc = open_dataset(file, name, &c.ds);
    if (rc != DRX_OK) goto out;
    rc = DRX_ERR_ARG;
    const hsize_t *dims = c.ds.dims, *chunk = c.ds.chunk;
    /* the padded last chunk is decoded into scratch (c.pad's plan and samples) and the rows that exist are copied out */
    const uint64_t n_full = dims[0] / chunk[0], edge_rows = dims[0] % chunk[0];
    s->rows = dims[0]; s->cols = dims[1]; s->chunk_rows = chunk[0]; s->n_chunks = n_full + (edge_rows ? 1 : 0);
    s->raw_bytes = dims[0] * dims[1] * 2;
    if (dims[0] * dims[1] > out_cap_samples) { rc = DRX_ERR_CAPACITY; goto out; }
    if (chunk[0] * chunk[1] > 0x7fffffffull) goto out;
    const uint32_t chunk_samples = (uint32_t)(chunk[0] * chunk[1]);

    /* sizes -> offsets -> the context's pinned staging buffer <- the stored chunks, slab by slab, each slab on its way to
     * the device while the next one is read */
    fx->h_off = (uint64_t *)malloc((s->n_chunks + 1) * sizeof(uint64_t));
    fx->h_addr = (uint64_t *)malloc((s->n_chunks + 1) * sizeof(uint64_t));
    if (!fx->h_off || !fx->h_addr) { rc = DRX_ERR_NOMEM; goto out; }
    int raw_ok;
    if ((rc = chunk_table(&c.ds, s->n_chunks, fx->h_off, fx->h_addr, &raw_ok)) != DRX_OK) goto out;
    const uint64_t words = fx->h_off[s->n_chunks];
    s->stored_bytes = words * 4;
    rc = DRX_ERR_NOMEM;
    if (drx_ctx_host_staging(ctx, words * 4, &h_words) != DRX_OK) goto out;
    if (hipMalloc(&fx->d_words, words * 4) != hipSuccess || hipMalloc((void **)&fx->d_off, (s->n_chunks + 1) * 8) != hipSuccess) goto out;
    slab_t slabs[kMaxSlabs];
    const int n_slabs = make_slabs(fx->h_off, s->n_chunks, slabs);
    const int raw_fd = raw_ok ? open(file, O_RDONLY | O_CLOEXEC) : -1;
    rc = raw_fd >= 0 ? fill_by_pread(raw_fd, fx, h_words, slabs, n_slabs, stream) : fill_by_read_chunk(&c.ds, fx, h_words, slabs, n_slabs, stream);
    if (rc != DRX_OK) goto out;
    s->t_file = now() - t0;

    t0 = now();
    rc = DRX_ERR_DEVICE;
    if (hipMemcpyAsync(fx->d_off, fx->h_off, (s->n_chunks + 1) * 8, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) goto out;
    s->t_pcie = now() - t0;  /* (what of the copies was left to wait for behind the last slab's read) */

    t0 = now();
    if (n_full) {
        if ((rc = source_plan(ctx, &c.ds, n_full, &c.plan)) != DRX_OK) goto out;
        if ((rc = drx_decode(c.plan, (const uint32_t *)fx->d_words, words, fx->d_off, d_out)) != DRX_OK) goto out;
        if ((rc = drx_plan_finish(c.plan, NULL)) != DRX_OK) goto out;
    }
    if (edge_rows) {
        if (hipMalloc(&c.pad.d_samples, (size_t)chunk_samples * 2) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
        if ((rc = source_plan(ctx, &c.ds, 1, &c.pad.plan)) != DRX_OK) goto out;
        if ((rc = drx_decode(c.pad.plan, (const uint32_t *)fx->d_words, words, fx->d_off + n_full, (int16_t *)c.pad.d_samples)) != DRX_OK) goto out;
        if ((rc = drx_plan_finish(c.pad.plan, NULL)) != DRX_OK) goto out;
        rc = DRX_ERR_DEVICE;
        if (hipMemcpyAsync(d_out + n_full * chunk_samples, c.pad.d_samples, (size_t)(edge_rows * dims[1]) * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) goto out;
    }
    rc = DRX_OK;
    s->t_gpu = now() - t0;
out:
    return call_release(&c, st, rc);
}

/* What drx_h5_read_rows, drx_h5_copy_rows and drx_h5_recompress fetch: the stored bytes of the chunks the rows lie in.
 * ds: an open dataset whose rows are wpr whole waveforms each; n_rows >= 1, every row below the dataset's.  s: the stats of what
 * was fetched, as far as it got. */
static drx_status fetch_rows_chunks(drx_ctx *ctx, const dataset_t *ds, const uint64_t *rows, uint64_t n_rows, uint64_t wpr,
                                    fetched_t *fx, drx_h5_stats *s) {
    const uint64_t chunk_rows = ds->chunk[0];
    void *h_words = NULL;  /* (the context's staging buffer, not freed here) */
    double t0 = now();
    fx->touched = (uint64_t *)malloc(n_rows * sizeof(uint64_t));
    fx->wave_idx = (uint64_t *)malloc(n_rows * wpr * sizeof(uint64_t));
    if (!fx->touched || !fx->wave_idx) return DRX_ERR_NOMEM;
    const uint64_t n_touched = s->n_chunks = fx->n_touched = touched_chunks(rows, n_rows, chunk_rows, fx->touched);
    /* their stored sizes -> offsets -> the context's staging buffer <- their stored bytes */
    uint64_t *h_off = fx->h_off = (uint64_t *)malloc((n_touched + 1) * sizeof(uint64_t));
    if (!h_off) return DRX_ERR_NOMEM;
    uint64_t words = 0;
    for (uint64_t t = 0; t < n_touched; ++t) {
        hsize_t off[2] = {fx->touched[t] * chunk_rows, 0}, nb = 0;
        if (H5Dget_chunk_storage_size(ds->d, off, &nb) < 0 || (nb & 3)) return DRX_ERR_CORRUPT;
        if (nb == 0) return DRX_ERR_UNSUPPORTED;  /* a chunk that was never written (fill value): not a stored stream */
        h_off[t] = words;
        words += nb / 4;
    }
    h_off[n_touched] = fx->words = words;
    s->stored_bytes = words * 4;
    if (drx_ctx_host_staging(ctx, words * 4, &h_words) != DRX_OK) return DRX_ERR_NOMEM;
    for (uint64_t t = 0; t < n_touched; ++t) {
        hsize_t off[2] = {fx->touched[t] * chunk_rows, 0};
        uint32_t mask = 0;
        if (H5Dread_chunk(ds->d, H5P_DEFAULT, off, &mask, (uint32_t *)h_words + h_off[t]) < 0 || mask) return DRX_ERR_CORRUPT;
    }
    s->t_file = now() - t0;

    t0 = now();
    hipStream_t stream = (hipStream_t)drx_ctx_stream(ctx);
    if (hipMalloc(&fx->d_words, words * 4) != hipSuccess || hipMalloc((void **)&fx->d_off, (n_touched + 1) * 8) != hipSuccess) return DRX_ERR_NOMEM;
    if (hipMemcpyAsync(fx->d_words, h_words, words * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(fx->d_off, h_off, (n_touched + 1) * 8, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) return DRX_ERR_DEVICE;
    s->t_pcie = now() - t0;

    rows_to_waves(rows, n_rows, chunk_rows, wpr, fx->touched, n_touched, fx->wave_idx);
    return DRX_OK;
}

drx_status drx_h5_read_rows(drx_ctx *ctx, const char *file, const char *name, const uint64_t *rows, uint64_t n_rows,
                            int16_t *d_out, uint64_t out_cap_samples, drx_h5_stats *st) {
    if (!ctx || !file || !name || (n_rows && (!rows || !d_out))) return DRX_ERR_ARG;
    call_t c;
    if (call_begin(&c, ctx) != 0) return DRX_ERR_DEVICE;
    const fetched_t *fx = &c.fx;
    drx_status rc = open_dataset(file, name, &c.ds);
    if (rc != DRX_OK) goto out;
    const uint64_t cols = c.ds.dims[1];
    uint64_t L, wpr;
    c.s.rows = c.ds.dims[0]; c.s.cols = cols; c.s.chunk_rows = c.ds.chunk[0];
    c.s.raw_bytes = n_rows * cols * 2;
    if ((rc = (drx_status)row_geometry(c.ds.dims[0], cols, c.ds.chunk[0], c.ds.o.wave_len, 0, rows, n_rows, &L, &wpr)) != DRX_OK) goto out;
    if (n_rows * cols > out_cap_samples) { rc = DRX_ERR_CAPACITY; goto out; }
    if (!n_rows) goto out;  /* (DRX_OK: the dataset's width is what the caller asked for) */

    if ((rc = fetch_rows_chunks(ctx, &c.ds, rows, n_rows, wpr, &c.fx, &c.s)) != DRX_OK) goto out;
    double t0 = now();
    if ((rc = source_plan(ctx, &c.ds, fx->n_touched, &c.plan)) != DRX_OK) goto out;
    if ((rc = drx_decode_select(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, fx->wave_idx, n_rows * wpr, d_out, L)) != DRX_OK) goto out;
    if ((rc = drx_plan_finish(c.plan, NULL)) != DRX_OK) goto out;
    c.s.t_gpu = now() - t0;
out:
    return call_release(&c, st, rc);
}

/* ---- the padded last chunk of a new dataset ---- */

/* The one-chunk plan (n_taps == 0: the delta filter), zeroed samples for the caller to put the rows into, room for the words. */
static drx_status pad_open(drx_ctx *ctx, padded_t *pad, uint32_t chunk_samples, uint32_t wave_len, unsigned k, unsigned n_taps, const int32_t *taps) {
    drx_status rc = drx_plan_create_uniform(ctx, 1, chunk_samples, wave_len, k, &pad->plan);
    if (rc == DRX_OK && n_taps) rc = drx_plan_set_filter(pad->plan, n_taps, taps);
    if (rc != DRX_OK) return rc;
    pad->cap = drx_plan_max_encoded_words(pad->plan);
    if (hipMalloc(&pad->d_samples, (size_t)chunk_samples * 2) != hipSuccess || hipMalloc(&pad->d_words, pad->cap * 4) != hipSuccess) return DRX_ERR_NOMEM;
    return hipMemsetAsync(pad->d_samples, 0, (size_t)chunk_samples * 2, (hipStream_t)drx_ctx_stream(ctx)) == hipSuccess ? DRX_OK : DRX_ERR_DEVICE;
}
/* d_off: the chunk's pair of offsets in the device's table (its words start at 0 of their own buffer) */
static drx_status pad_encode(padded_t *pad, uint64_t *d_off) {
    return drx_encode(pad->plan, (const int16_t *)pad->d_samples, (uint32_t *)pad->d_words, pad->cap, d_off);
}
static drx_status pad_finish(padded_t *pad) { return drx_plan_finish(pad->plan, &pad->words); }
/* Behind n_full chunks of `words` words in h_off / h_words: the chunk's end among the offsets (h_off[n_full] is `words`, or the
 * 0 of h_off[0] without full chunks), and its words on their way to the host. */
static void pad_splice(const padded_t *pad, uint64_t *h_off, uint64_t n_full, uint64_t words) { h_off[n_full + 1] = words + pad->words; }
static int pad_copy_out(const padded_t *pad, void *h_words, uint64_t words, hipStream_t stream) {
    return hipMemcpyAsync((uint32_t *)h_words + words, pad->d_words, pad->words * 4, hipMemcpyDeviceToHost, stream) == hipSuccess ? 0 : -1;
}

/* The result to the host: n chunks of `words` words, and pad's chunk behind them if pad is not NULL: the offsets to res->h_off
 * and the words to the context's staging buffer *h_words (the fetched bytes have left it). */
static drx_status result_to_host(drx_ctx *ctx, result_t *res, uint64_t n, uint64_t words, const padded_t *pad, void **h_words) {
    hipStream_t stream = (hipStream_t)drx_ctx_stream(ctx);
    res->h_off = (uint64_t *)malloc((n + 3) * 8);
    if (!res->h_off || drx_ctx_host_staging(ctx, (words + (pad ? pad->words : 0) + 1) * 4, h_words) != DRX_OK) return DRX_ERR_NOMEM;
    res->h_off[0] = 0;
    if (n && (hipMemcpyAsync(res->h_off, res->d_off, (n + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
              hipMemcpyAsync(*h_words, res->d_words, words * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)) return DRX_ERR_DEVICE;
    if (pad && pad_copy_out(pad, *h_words, words, stream) != 0) return DRX_ERR_DEVICE;
    if (hipStreamSynchronize(stream) != hipSuccess) return DRX_ERR_DEVICE;
    if (pad) pad_splice(pad, res->h_off, n, words);
    return DRX_OK;
}

/* A new file with one dataset of filter 32025, written with H5Dwrite_chunk. */
typedef struct { hid_t f, d; const char *file; uint64_t chunk_rows; } dst_t;
/* file (created / truncated), space, property list with chunking and the filter, dataset of element type `type`.  On failure
 * whatever was opened is left for dst_close(). */
static drx_status dst_create(dst_t *dst, const char *name, hid_t type, uint64_t rows, uint64_t cols, unsigned flags, size_t ncd, const unsigned *cd) {
    ensure_filter_registered();
    if (type < 0 || (dst->f = H5Fcreate(dst->file, H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT)) < 0) return DRX_ERR_ARG;
    hsize_t dims[2] = {rows, cols}, chunk[2] = {dst->chunk_rows, cols};
    const hid_t sp = H5Screate_simple(2, dims, NULL), pl = H5Pcreate(H5P_DATASET_CREATE);
    if (H5Pset_chunk(pl, 2, chunk) >= 0 && H5Pset_filter(pl, FILTER_ID, flags, ncd, cd) >= 0)
        dst->d = H5Dcreate2(dst->f, name, type, sp, H5P_DEFAULT, pl, H5P_DEFAULT);
    if (pl >= 0) H5Pclose(pl);
    if (sp >= 0) H5Sclose(sp);
    return dst->d < 0 ? DRX_ERR_ARG : DRX_OK;
}
/* chunks [c0, c1) from their offsets and the words */
static drx_status dst_write_chunks(dst_t *dst, uint64_t c0, uint64_t c1, const uint64_t *h_off, const void *h_words) {
    for (uint64_t c = c0; c < c1; ++c) {
        hsize_t off[2] = {c * dst->chunk_rows, 0};
        if (H5Dwrite_chunk(dst->d, H5P_DEFAULT, 0, off, (size_t)(h_off[c + 1] - h_off[c]) * 4, (const uint32_t *)h_words + h_off[c]) < 0) return DRX_ERR_ARG;
    }
    return DRX_OK;
}
/* rc: the call's status so far -> the call's status: a file that does not close is DRX_ERR_ARG.  unlink_failed: no half-written
 * file is left behind. */
static drx_status dst_close(dst_t *dst, drx_status rc, int unlink_failed) {
    if (dst->d >= 0) H5Dclose(dst->d);
    if (dst->f >= 0) {
        if (H5Fclose(dst->f) < 0 && rc == DRX_OK) rc = DRX_ERR_ARG;
        if (rc != DRX_OK && unlink_failed) (void)unlink(dst->file);
    }
    dst->f = dst->d = -1;
    return rc;
}
/* All three for a file-to-file call, which has every chunk in the staging buffer: a dataset of the source's element type and
 * filter flags with the cd_values given. */
static drx_status dst_store(const char *file, const char *name, const dataset_t *src, uint64_t rows, uint64_t chunk_rows, size_t ncd, const unsigned *cd,
                            uint64_t n_chunks, const uint64_t *h_off, const void *h_words, drx_h5_stats *s) {
    const double t0 = now();
    dst_t dst = {-1, -1, file, chunk_rows};
    drx_status rc = dst_create(&dst, name, src->ty, rows, src->dims[1], src->flags, ncd, cd);
    if (rc == DRX_OK) rc = dst_write_chunks(&dst, 0, n_chunks, h_off, h_words);
    rc = dst_close(&dst, rc, 1);
    s->t_file += now() - t0;
    return rc;
}

/* File -> file: rows of one dataset into a new dataset of another file, the gathered chunks never decoded. */
drx_status drx_h5_copy_rows(drx_ctx *ctx, const char *src_file, const char *src_name, const uint64_t *rows, uint64_t n_rows,
                            const char *dst_file, const char *dst_name, uint64_t dst_chunk_rows, drx_h5_stats *st) {
    if (!ctx || !src_file || !src_name || !dst_file || !dst_name || !rows || !n_rows || dst_chunk_rows > n_rows)
        return DRX_ERR_ARG;  /* (HDF5: chunk <= dataset) */
    if (same_file(src_file, dst_file)) return DRX_ERR_ARG;
    call_t c;
    if (call_begin(&c, ctx) != 0) return DRX_ERR_DEVICE;
    const dataset_t *ds = &c.ds;
    const fetched_t *fx = &c.fx;
    void *h_words = NULL;
    drx_status rc = open_dataset(src_file, src_name, &c.ds);
    if (rc != DRX_OK) goto out;
    const uint64_t cols = ds->dims[1], chunk_rows = ds->chunk[0];
    uint64_t L, wpr;
    if (!dst_chunk_rows) dst_chunk_rows = chunk_rows < n_rows ? chunk_rows : n_rows;  /* the source's chunking */
    c.s.rows = n_rows; c.s.cols = cols; c.s.chunk_rows = dst_chunk_rows;
    c.s.raw_bytes = n_rows * cols * 2;
    if ((rc = (drx_status)row_geometry(ds->dims[0], cols, chunk_rows, ds->o.wave_len, dst_chunk_rows, rows, n_rows, &L, &wpr)) != DRX_OK) goto out;
    if ((rc = fetch_rows_chunks(ctx, ds, rows, n_rows, wpr, &c.fx, &c.s)) != DRX_OK) goto out;

    /* whole output chunks: one gather, sized first.  Rows left over: the padded last chunk, those rows decoded into it */
    double t0 = now();
    const uint64_t n_full = n_rows / dst_chunk_rows, edge_rows = n_rows % dst_chunk_rows, n_out = n_full + (edge_rows ? 1 : 0);
    const uint64_t n_sel = n_full * dst_chunk_rows * wpr;
    uint64_t words = 0;
    if ((rc = source_plan(ctx, ds, fx->n_touched, &c.plan)) != DRX_OK) goto out;
    if (hipMalloc((void **)&c.res.d_off, (n_out + 3) * 8) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
    if (n_full) {
        if ((rc = drx_gather_encoded(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, fx->wave_idx, n_sel, dst_chunk_rows * wpr,
                                     NULL, 0, c.res.d_off, NULL)) != DRX_OK) goto out;
        if ((rc = drx_plan_finish(c.plan, &words)) != DRX_OK) goto out;
        if (hipMalloc(&c.res.d_words, words * 4) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
        if ((rc = drx_gather_encoded(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, fx->wave_idx, n_sel, dst_chunk_rows * wpr,
                                     (uint32_t *)c.res.d_words, words, c.res.d_off, NULL)) != DRX_OK) goto out;
        if ((rc = drx_plan_finish(c.plan, &words)) != DRX_OK) goto out;
    }
    if (edge_rows) {
        if ((rc = pad_open(ctx, &c.pad, (uint32_t)(dst_chunk_rows * cols), (uint32_t)L, ds->o.rice_k, ds->o.n_taps, ds->o.taps)) != DRX_OK) goto out;
        if ((rc = drx_decode_select(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, fx->wave_idx + n_sel, edge_rows * wpr,
                                    (int16_t *)c.pad.d_samples, L)) != DRX_OK) goto out;
        if ((rc = drx_plan_finish(c.plan, NULL)) != DRX_OK) goto out;
        if ((rc = pad_encode(&c.pad, c.res.d_off + n_full + 1)) != DRX_OK || (rc = pad_finish(&c.pad)) != DRX_OK) goto out;
    }
    c.s.t_gpu = now() - t0;

    t0 = now();
    if ((rc = result_to_host(ctx, &c.res, n_full, words, edge_rows ? &c.pad : NULL, &h_words)) != DRX_OK) goto out;
    c.s.t_pcie += now() - t0;
    /* the new dataset: the source's element type and cd_values verbatim, chunks of dst_chunk_rows x cols */
    rc = dst_store(dst_file, dst_name, ds, n_rows, dst_chunk_rows, ds->ncd, ds->cd, n_out, c.res.h_off, h_words, &c.s);
out:
    return call_release(&c, st, rc);
}

/* File -> file: every stored chunk of one dataset re-coded at another RiceParameter, never decoded. */
drx_status drx_h5_recompress(drx_ctx *ctx, const char *src_file, const char *src_name, const char *dst_file, const char *dst_name,
                             unsigned rice_m, drx_h5_stats *st) {
    return drx_h5_recompress_filtered(ctx, src_file, src_name, dst_file, dst_name, rice_m, 0, NULL, st);
}

/* ... and, with n_taps != 0, under another prediction filter (drx_transcode_filter): never decoded to memory. */
drx_status drx_h5_recompress_filtered(drx_ctx *ctx, const char *src_file, const char *src_name, const char *dst_file, const char *dst_name,
                                      unsigned rice_m, unsigned n_taps, const int32_t *taps, drx_h5_stats *st) {
    if (!ctx || !src_file || !src_name || !dst_file || !dst_name) return DRX_ERR_ARG;
    if (n_taps > DRX_MAX_TAPS || (n_taps && (!taps || taps[0] == 0))) return DRX_ERR_ARG;
    unsigned k2 = 0;
    if (rice_m && log2_m(rice_m, &k2)) return DRX_ERR_ARG;
    if (same_file(src_file, dst_file)) return DRX_ERR_ARG;
    call_t c;
    if (call_begin(&c, ctx) != 0) return DRX_ERR_DEVICE;
    dataset_t *ds = &c.ds;
    const fetched_t *fx = &c.fx;
    void *h_words = NULL;
    drx_status rc = open_dataset(src_file, src_name, ds);
    if (rc != DRX_OK) goto out;
    rc = DRX_ERR_ARG;
    const uint64_t n_data_rows = ds->dims[0], cols = ds->dims[1], chunk_rows = ds->chunk[0];
    if (!n_data_rows || chunk_rows * cols > 0x7fffffffull) goto out;
    /* HDF5 stores a last chunk that the rows do not fill at full size: every stored chunk has one geometry */
    const uint64_t n_chunks = (n_data_rows + chunk_rows - 1) / chunk_rows;
    c.s.rows = n_data_rows; c.s.cols = cols; c.s.chunk_rows = chunk_rows;
    c.s.raw_bytes = n_data_rows * cols * 2;

    /* every stored chunk to the staging buffer and to the device: the first row of each names it */
    if (!(c.rows = (uint64_t *)malloc(n_chunks * sizeof(uint64_t)))) { rc = DRX_ERR_NOMEM; goto out; }
    for (uint64_t i = 0; i < n_chunks; ++i) c.rows[i] = i * chunk_rows;
    if ((rc = fetch_rows_chunks(ctx, ds, c.rows, n_chunks, 1, &c.fx, &c.s)) != DRX_OK) goto out;

    /* one estimate where the best parameter is asked for (it gives the result's size too), one transcode */
    double t0 = now();
    uint64_t words = 0, cap = 0;
    if ((rc = source_plan(ctx, ds, n_chunks, &c.plan)) != DRX_OK) goto out;
    if (!rice_m) {
        uint64_t est[16];
        rc = n_taps ? drx_estimate_words_encoded_filter(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, NULL, n_taps, taps, est)
                    : drx_estimate_words_encoded(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, NULL, est);
        if (rc != DRX_OK) goto out;
        for (unsigned k = 1; k < 16; ++k) if (est[k] < est[k2]) k2 = k;  /* (on a tie the smaller) */
        cap = est[k2];
    } else {
        cap = drx_plan_max_encoded_words(c.plan);
    }
    if (hipMalloc(&c.res.d_words, cap * 4) != hipSuccess || hipMalloc((void **)&c.res.d_off, (n_chunks + 1) * 8) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
    rc = n_taps ? drx_transcode_filter(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, k2, n_taps, taps, (uint32_t *)c.res.d_words, cap, c.res.d_off, NULL)
                : drx_transcode(c.plan, (const uint32_t *)fx->d_words, fx->words, fx->d_off, k2, (uint32_t *)c.res.d_words, cap, c.res.d_off, NULL);
    if (rc != DRX_OK) goto out;
    if ((rc = drx_plan_finish(c.plan, &words)) != DRX_OK) goto out;
    c.s.t_gpu = now() - t0;

    t0 = now();
    if ((rc = result_to_host(ctx, &c.res, n_chunks, words, NULL, &h_words)) != DRX_OK) goto out;
    c.s.t_pcie += now() - t0;
    /* the new dataset: the source's shape, element type and chunking, its cd_values but for the RiceParameter and the new taps */
    const size_t ncd = recompress_cd_values(ds->ncd, ds->cd, 1u << k2, ds->o.wave_len, n_taps, taps);
    rc = dst_store(dst_file, dst_name, ds, n_data_rows, chunk_rows, ncd, ds->cd, n_chunks, c.res.h_off, h_words, &c.s);
out:
    return call_release(&c, st, rc);
}

/* drx_h5_write's copies on the copy stream: an error path may leave some in flight into the staging buffer and out of the device
 * buffers, so the stream is synchronised before the events are destroyed and the buffers freed. */
static void drain_copies(hipStream_t cs, hipEvent_t *ev, int n_ev) {
    if (n_ev) (void)hipStreamSynchronize(cs);
    for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
}

drx_status drx_h5_write(drx_ctx *ctx, const char *file, const char *name, const int16_t *d_in,
                        uint64_t rows, uint64_t cols, uint64_t chunk_rows, unsigned rice_m,
                        unsigned wave_len, drx_h5_stats *st) {
    return drx_h5_write_filtered(ctx, file, name, d_in, rows, cols, chunk_rows, rice_m, wave_len, 0, NULL, st);
}

drx_status drx_h5_write_filtered(drx_ctx *ctx, const char *file, const char *name, const int16_t *d_in,
                                 uint64_t rows, uint64_t cols, uint64_t chunk_rows, unsigned rice_m,
                                 unsigned wave_len, unsigned n_taps, const int32_t *taps, drx_h5_stats *st) {
    if (!ctx || !file || !name || !d_in || !rows || !cols || !chunk_rows || chunk_rows > rows) return DRX_ERR_ARG;  /* HDF5: chunk <= dataset */
    if (n_taps > DRX_MAX_TAPS || (n_taps && !taps)) return DRX_ERR_ARG;
    unsigned k;
    if (log2_m(rice_m, &k) || chunk_rows * cols > 0x7fffffffull) return DRX_ERR_ARG;
    call_t c;
    if (call_begin(&c, ctx) != 0) return DRX_ERR_DEVICE;
    drx_h5_stats *s = &c.s;
    result_t *res = &c.res;  /* (the full chunks' words and every chunk's offsets; the padded last chunk is c.pad) */
    /* rows that do not divide: the padded last chunk */
    const uint64_t n_full = rows / chunk_rows, edge_rows = rows % chunk_rows;
    const uint32_t chunk_samples = (uint32_t)(chunk_rows * cols);
    s->rows = rows; s->cols = cols; s->chunk_rows = chunk_rows; s->n_chunks = n_full + (edge_rows ? 1 : 0);
    s->raw_bytes = rows * cols * 2;
    drx_status rc = DRX_ERR_DEVICE;
    dst_t dst = {-1, -1, file, chunk_rows};
    void *h_words = NULL;  /* (the context's staging buffer, not freed here) */
    hipStream_t stream = (hipStream_t)drx_ctx_stream(ctx), cs = stream;

    double t0 = now();
    uint64_t words = 0, cap = 0;
    hipEvent_t ev[kMaxSlabs];
    int n_ev = 0;
    if (hipMalloc((void **)&res->d_off, (s->n_chunks + 3) * 8) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
    /* the encoders are launched ... */
    if (n_full) {
        if ((rc = drx_plan_create_uniform(ctx, n_full, chunk_samples, wave_len, k, &c.plan)) != DRX_OK) goto out;
        if (n_taps && (rc = drx_plan_set_filter(c.plan, n_taps, taps)) != DRX_OK) goto out;
        cap = drx_plan_max_encoded_words(c.plan);
        if (hipMalloc(&res->d_words, cap * 4) != hipSuccess) { rc = DRX_ERR_NOMEM; goto out; }
        if ((rc = drx_encode(c.plan, d_in, (uint32_t *)res->d_words, cap, res->d_off)) != DRX_OK) goto out;
    }
    if (edge_rows) {
        if ((rc = pad_open(ctx, &c.pad, chunk_samples, wave_len, k, n_taps, taps)) != DRX_OK) goto out;
        if (hipMemcpyAsync(c.pad.d_samples, d_in + n_full * chunk_samples, (size_t)(edge_rows * cols) * 2, hipMemcpyDeviceToDevice, stream) != hipSuccess) { rc = DRX_ERR_DEVICE; goto out; }
        if ((rc = pad_encode(&c.pad, res->d_off + n_full + 1)) != DRX_OK) goto out;
    }
    /* ... and run while the file and the dataset are created */
    double t1 = now();
    unsigned cd[3 + DRX_MAX_TAPS];  /* src/deltaRice.c:248-291 */
    const size_t ncd = write_cd_values(rice_m, wave_len, n_taps, taps, cd);
    if ((rc = dst_create(&dst, name, H5T_NATIVE_SHORT, rows, cols, H5Z_FLAG_MANDATORY, ncd, cd)) != DRX_OK) goto out;
    s->t_file = now() - t1;
    t1 = now();
    if (n_full && (rc = drx_plan_finish(c.plan, &words)) != DRX_OK) goto out;
    if (edge_rows && (rc = pad_finish(&c.pad)) != DRX_OK) goto out;
    s->t_gpu = (t1 - t0 - s->t_file) + (now() - t1);  /* launches + what was left of the kernels behind the file's creation */
    s->stored_bytes = (words + c.pad.words) * 4;

    /* chunk offsets, then the chunks themselves slab by slab on the copy stream into the context's pinned staging buffer,
     * each slab written to the file (H5Dwrite_chunk) while the slabs behind it cross PCIe */
    t0 = now();
    rc = DRX_ERR_NOMEM;
    uint64_t *h_off = res->h_off = (uint64_t *)malloc((s->n_chunks + 3) * 8);
    if (!h_off || drx_ctx_host_staging(ctx, (words + c.pad.words + 1) * 4, &h_words) != DRX_OK) goto out;
    rc = DRX_ERR_DEVICE;
    h_off[0] = 0;
    if (n_full && (hipMemcpyAsync(h_off, res->d_off, (n_full + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)) goto out;
    if (edge_rows) pad_splice(&c.pad, h_off, n_full, words);
    if (copy_stream_of(drx_ctx_device(ctx))) cs = copy_stream_of(drx_ctx_device(ctx));
    slab_t slabs[kMaxSlabs];
    const int n_slabs = make_slabs(h_off, s->n_chunks, slabs);
    for (int sl = 0; sl < n_slabs; ++sl) {
        /* (the padded chunk, if any, is the last chunk and lies in its own device buffer) */
        const uint64_t c0 = slabs[sl].c0, c1 = slabs[sl].c1 > n_full ? n_full : slabs[sl].c1;
        if (c0 < c1 && hipMemcpyAsync((uint32_t *)h_words + h_off[c0], (const uint32_t *)res->d_words + h_off[c0], (h_off[c1] - h_off[c0]) * 4,
                                      hipMemcpyDeviceToHost, cs) != hipSuccess) goto out;
        if (slabs[sl].c1 > n_full && pad_copy_out(&c.pad, h_words, words, cs) != 0) goto out;
        if (hipEventCreateWithFlags(&ev[n_ev], hipEventDisableTiming) != hipSuccess) goto out;
        ++n_ev;
        if (hipEventRecord(ev[n_ev - 1], cs) != hipSuccess) goto out;
    }
    double t_wait = now() - t0, t_h5 = 0;
    for (int sl = 0; sl < n_slabs; ++sl) {
        t1 = now();
        if (hipEventSynchronize(ev[sl]) != hipSuccess) goto out;
        t_wait += now() - t1;
        t1 = now();
        if ((rc = dst_write_chunks(&dst, slabs[sl].c0, slabs[sl].c1, h_off, h_words)) != DRX_OK) goto out;
        rc = DRX_ERR_DEVICE;
        t_h5 += now() - t1;
    }
    s->t_pcie = t_wait;  /* (the copies the calling thread had to WAIT for; the rest ran under H5Dwrite_chunk) */
    s->t_file += t_h5;
    t0 = now();
    rc = DRX_OK;
out:
    rc = dst_close(&dst, rc, 0);  /* (a failed write leaves the file as far as it got) */
    if (rc == DRX_OK) s->t_file += now() - t0;  /* (closing the dataset and the file) */
    drain_copies(cs, ev, n_ev);
    return call_release(&c, st, rc);
}
