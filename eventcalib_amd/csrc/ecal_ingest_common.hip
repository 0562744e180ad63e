// What the host sides of the ingests share (ecal_ctx.hpp declares it): the refusals of a device form's arguments, the counters'
// wipe and fetch, the record buffer an ingest allocates for its caller, the full read, the windowed reader and the front of the file
// forms, their middle that indexes a file beside its upload (bag, MCAP, AEDAT 3.1, AEDAT 4), and the two ends of every file form (a
// stream, a .bin file).  The drivers that are templates over a format's kernels are ingest_driver.hpp's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ecal_ctx.hpp"

int ecal_ingest_check_buffer(ecal_ctx *ctx, const char *who, const void *ptr, uint64_t n, uint32_t align, const char *what,
                             const char *what_aligned, const char *plural) {
    if (n && !ptr) {
        ctx->last_error = std::string(who) + ": null " + what;
        return ECAL_ERR_INVALID;
    }
    if ((uintptr_t) ptr & (align - 1u)) {
        ctx->last_error = std::string(who) + ": the " + (what_aligned ? what_aligned : what) + " must be " + std::to_string(align) + "-byte aligned";
        return ECAL_ERR_INVALID;
    }
    if (plural && n > 0x7FFFFFFFull) {
        ctx->last_error = std::string(who) + ": more than 2^31-1 " + plural;
        return ECAL_ERR_RANGE;
    }
    return ECAL_OK;
}

int ecal_ingest_wipe_words(ecal_ctx *ctx, void *d_words, size_t bytes, unsigned long long *d_none, hipStream_t st) {
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_words, 0, bytes, st));
    ECAL_HIP_TRY(ctx, hipMemsetAsync(d_none, 0xFF, sizeof(unsigned long long), st));
    return ECAL_OK;
}

int ecal_ingest_fetch_words(ecal_ctx *ctx, void *words, const void *d_words, size_t bytes, hipStream_t st) {
    ECAL_HIP_TRY(ctx, hipMemcpyAsync(words, d_words, bytes, hipMemcpyDeviceToHost, st));
    ECAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    return ECAL_OK;
}

int ecal_ingest_alloc_records(ecal_ctx *ctx, const char *who, uint64_t n, uint8_t **own) {
    hipError_t e = hipMalloc((void **) own, (size_t) n * 25 + 16);
    if (e != hipSuccess) {
        *own = nullptr;
        ctx->last_error = std::string(who) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
    }
    return ECAL_OK;
}

int ecal_ingest_drop_records(uint8_t **own, int code) {
    if (own && *own) {
        (void) hipFree(*own);
        *own = nullptr;
    }
    return code;
}

bool ecal_ingest_pread_all(int fd, void *dst, size_t n, uint64_t at) {
    for (size_t got = 0; got < n;) {
        const ssize_t rd = pread(fd, (uint8_t *) dst + got, n - got, (off_t) (at + got));
        if (rd <= 0) return false;
        got += (size_t) rd;
    }
    return true;
}

bool ecal_ingest_file_reader::operator()(uint64_t pos, uint8_t *dst, size_t n) {
    if (pos >= win_at && pos + n <= win_at + win_n) {
        memcpy(dst, win.data() + (pos - win_at), n);
        return true;
    }
    if (n >= WINDOW) return ecal_ingest_pread_all(fd, dst, n, pos);
    const size_t want = (size_t) std::min<uint64_t>(WINDOW, file_bytes - pos);
    win.resize(WINDOW);
    if (!ecal_ingest_pread_all(fd, win.data(), want, pos)) return false;
    win_at = pos;
    win_n = want;
    memcpy(dst, win.data(), n);
    return true;
}

int ecal_ingest_open_head(ecal_ctx *ctx, const char *who, const char *path, size_t head_max, const char *unread, int *fd, uint64_t *file_bytes,
                          std::vector<uint8_t> *head) {
    *fd = open(path, O_RDONLY);
    if (*fd < 0) {
        ctx->last_error = std::string(who) + ": cannot open " + path;
        return ECAL_ERR_INVALID;
    }
    struct stat sb;
    const bool sized = fstat(*fd, &sb) == 0;
    if (sized) {
        *file_bytes = (uint64_t) sb.st_size;
        head->resize((size_t) std::min<uint64_t>(*file_bytes, head_max));
    }
    if (!sized || !ecal_ingest_pread_all(*fd, head->data(), head->size(), 0)) {
        close(*fd);
        *fd = -1;
        ctx->last_error = sized && unread ? std::string(who) + ": " + unread + " (" + path + ")" : std::string(who) + ": cannot read " + path;
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

int ecal_ingest_upload_indexed(ecal_ctx *ctx, const char *tag, const char *who, const char *index_label, const char *path, int fd,
                               uint64_t file_offset, uint64_t expect_bytes, const ecal_ingest_index_fn &index, ecal_ingest_upload *up) {
    typedef std::chrono::steady_clock clock;
    auto ms_since = [](clock::time_point t) { return 1e3 * std::chrono::duration<double>(clock::now() - t).count(); };
    *up = ecal_ingest_upload();
    const void *table = nullptr;
    size_t table_bytes = 0;
    int index_rc = ECAL_OK;
    std::string index_error;
    double index_ms = 0;
    std::thread indexer;
    if (index)
        indexer = std::thread([&]() {   // nothing of the context is touched on this thread: index_error takes the text
            const auto t0 = clock::now();
            index_rc = index(&index_error, &table, &table_bytes);
            index_ms = ms_since(t0);
        });
    const auto t0 = clock::now();
    int rc = hipSetDevice(ctx->device) == hipSuccess ? ECAL_OK : ECAL_ERR_HIP;
    if (rc) ctx->last_error = std::string(who) + ": hipSetDevice failed";
    else rc = ecal_upload_file(ctx, who, path, file_offset, &up->d_file, &up->n_bytes);
    const double upload_ms = ms_since(t0);
    if (indexer.joinable()) indexer.join();
    close(fd);
    if (!rc && index_rc) {
        rc = index_rc;
        ctx->last_error = index_error;
    }
    if (!rc && expect_bytes != ECAL_INGEST_ANY_SIZE && up->n_bytes != expect_bytes) {
        rc = ECAL_ERR_INVALID;
        ctx->last_error = std::string(who) + ": the file changed while it was read (" + path + ")";
    }
    if (rc) {
        if (up->d_file) (void) hipFree(up->d_file);
        *up = ecal_ingest_upload();
        return rc;
    }
    if (ctx->sw.load_trace) {
        if (index) fprintf(stderr, "ecal %s ingest: %-24s %.3f ms\n", tag, index_label, index_ms);
        fprintf(stderr, "ecal %s ingest: %-24s %.3f ms\n", tag, "file read + upload", upload_ms);
        fprintf(stderr, "ecal %s ingest: %-24s %.3f ms\n", tag, "index beside upload", ms_since(t0));
    }
    if (table_bytes) {
        hipError_t e = hipMalloc(&up->d_table, table_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(up->d_table, table, table_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            ctx->last_error = std::string(who) + ": " + hipGetErrorString(e);
            ecal_ingest_free_upload(ctx, up);
            return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
        }
    }
    return ECAL_OK;
}

void ecal_ingest_free_upload(ecal_ctx *ctx, ecal_ingest_upload *up) {
    (void) hipStreamSynchronize(ctx->stream);   // (the table's upload reads host memory that its owner may drop behind this)
    if (up->d_table) (void) hipFree(up->d_table);
    if (up->d_file) (void) hipFree(up->d_file);
    *up = ecal_ingest_upload();
}

int ecal_stream_from_events(ecal_ctx *ctx, const char *who, uint8_t *d_events, uint64_t n_events, ecal_stream **out) {
    if (!d_events) {   // no events: a stream of none
        hipError_t e = hipMalloc((void **) &d_events, 16);
        if (e != hipSuccess) {
            ctx->last_error = std::string(who) + ": " + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? ECAL_ERR_NOMEM : ECAL_ERR_HIP;
        }
    }
    return ecal_stream_adopt(ctx, d_events, n_events, out);
}

int ecal_ingest_records_to_bin(ecal_ctx *ctx, const char *who, uint8_t *d_events, uint64_t n_events, const char *bin_path) {
    const int rc = ecal_write_records_file(ctx, who, d_events, n_events, bin_path);
    if (d_events) (void) hipFree(d_events);
    return rc;
}
