// The host drivers the table ingests share (ecal_bag.hip, ecal_mcap.hip, ecal_aedat.hip, ecal_aedat4.hip), templates over the format's
// counters and kernel launches; what is no template is ecal_ingest_common.hip's (ecal_ctx.hpp).
//   ecal_ingest_scan_table      the one-workgroup scan of a table alone, its counters on the host
//   ecal_ingest_verdict_write   the back half of every ingest: verdict -> block scan -> write -> fetch -> counters -> capacity
//   ecal_ingest_message_table   the whole device path of a message (or packet) table: bag, MCAP STRUCT / MONO, AEDAT 3.1
#pragma once
#include <algorithm>
#include <string>
#include "ecal_ctx.hpp"

// the texts of a message-table ingest: who opens the errors, tag names the trace lines, entry / holder are the nouns of the refusals
// ("message" / "file", "packet" / "payload"), scan_mark labels the table scan's phase
struct ecal_ingest_nouns {
    const char *who, *tag, *entry, *holder, *scan_mark;
};

// first[0, n] = the scan of the table, by launch_scan(first, d_w), in `scratch` (the counters behind it), and the counters in W: one look
// at them.  "<who>: <k> <entry>s of the table do not lie within the <holder>" + bad_suffix when W.bad_table
template <class Words, class LaunchScan>
int ecal_ingest_scan_table(ecal_ctx *ctx, const ecal_ingest_nouns &N, uint64_t n_entries, ecal_devbuf &scratch, Words &W, const char *bad_suffix,
                           hipStream_t st, LaunchScan launch_scan) {
    const size_t o_words = up16((size_t) (n_entries + 1) * 8);
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, o_words + sizeof(Words)))) return rc;
    Words *d_w = (Words *) (scratch.as<uint8_t>() + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(Words), &d_w->first_stop, st))) return rc;
    launch_scan(scratch.as<unsigned long long>(), d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return rc;
    if (W.bad_table) {
        ctx->last_error = std::string(N.who) + ": " + std::to_string(W.bad_table) + " " + N.entry + "s of the table do not lie within the " + N.holder + bad_suffix;
        return ECAL_ERR_INVALID;
    }
    return ECAL_OK;
}

// The back half: launch_verdict() over nb blocks into keep, ecal_scan_blocks into koff, launch_write(), the counters fetched (the one
// look behind the write), after(W, &n_more) — the format's own checks and fields; n_more: events of a class that only it counts
// (AEDAT's n_invalid); non-zero ends the ingest —, then I's counters, n_after_end and the capacity refusal.  I.n_raw_events is set by
// the caller or by after.  The buffer of own_events (may be null) is dropped on every failure.
template <class Words, class Info, class LaunchVerdict, class LaunchWrite, class After>
int ecal_ingest_verdict_write(ecal_ctx *ctx, const char *who, ecal_load_timer &tm, uint32_t nb, uint32_t *keep, uint32_t *koff, const Words *d_w,
                              uint64_t capacity, uint8_t **own_events, Info &I, hipStream_t st, LaunchVerdict launch_verdict, LaunchWrite launch_write,
                              After after) {
    auto fail = [&](int code) { return ecal_ingest_drop_records(own_events, code); };
    auto launched = [&]() -> int {
        ECAL_HIP_TRY(ctx, hipGetLastError());
        return ECAL_OK;
    };
    int rc;
    launch_verdict();
    if ((rc = launched())) return fail(rc);
    tm.mark("verdict");
    if ((rc = ecal_scan_blocks(ctx, keep, nb, koff, st))) return fail(rc);
    launch_write();
    if ((rc = launched())) return fail(rc);
    tm.mark("scan, write");
    Words W;
    if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return fail(rc);
    uint64_t n_more = 0;
    if ((rc = after(W, &n_more))) return fail(rc);
    I.n_events = W.n_events;
    I.n_outside = W.n_outside;
    I.n_negative = W.n_negative;
    I.n_before_start = W.n_before_start;
    // every event in front of the offender has one of the classes
    I.n_after_end = W.first_stop == ~0ull ? 0 : I.n_raw_events - (W.n_events + n_more + W.n_outside + W.n_negative + W.n_before_start);
    if (I.n_events > capacity) {
        ctx->last_error = std::string(who) + ": " + std::to_string(I.n_events) + " records, more than the capacity";
        return fail(ECAL_ERR_RANGE);
    }
    return ECAL_OK;
}

// A table of n_entries messages over n_bytes into records.  src: the format's source with the file and the table in it; its `first`
// and `n_slots` are set here.  event_bytes: no event takes fewer (sizes the per-block arrays when the slots are not known).
// n_slots_host: the sum of the table's counts when the caller knows it (the file forms), else all ones: then the host looks at the
// scan once, the grid being a count of the table.
// own_events != null: the records go into a buffer allocated here for the count (the caller's to hipFree, null when there is nothing
// to free); else into d_events / capacity.
// launch_scan(first, d_w), launch_verdict(src, flt, nb, keep, d_w), launch_write(src, flt, nb, koff, d_events, capacity, d_w): the
// format's kernels; after(W, &n_more): as above, behind the table's own check.
template <class Words, class Source, class Filter, class Info, class LaunchScan, class LaunchVerdict, class LaunchWrite, class After>
int ecal_ingest_message_table(ecal_ctx *ctx, const ecal_ingest_nouns &N, Source src, const Filter &flt, uint64_t n_bytes, uint64_t n_entries,
                              uint64_t event_bytes, uint64_t n_slots_host, uint32_t block_events, uint8_t *d_events, uint64_t capacity,
                              uint8_t **own_events, Info &I, hipStream_t st, LaunchScan launch_scan, LaunchVerdict launch_verdict,
                              LaunchWrite launch_write, After after) {
    constexpr uint64_t NONE = ~0ull;
    const std::string who = N.who, entry = N.entry, holder = N.holder;
    if (own_events) *own_events = nullptr;
    if (!n_entries || n_slots_host == 0) return ECAL_OK;
    // no fewer than the slots: sizes the per-block arrays
    const uint64_t bound = n_slots_host != NONE ? n_slots_host : std::min<uint64_t>(n_bytes / event_bytes, 0xFFFFFFFFull);
    if (bound > 0xFFFFFFFFull) {
        I.n_events = bound;
        ctx->last_error = who + ": more than 2^32-1 events";
        return ECAL_ERR_RANGE;
    }
    const uint32_t nb_max = (uint32_t) ((bound + block_events - 1) / block_events);
    ecal_load_timer tm(N.tag, ctx->sw.load_trace, st);
    const size_t o_first = 0, o_keep = o_first + up16((size_t) (n_entries + 1) * 8), o_koff = o_keep + up16(((size_t) nb_max + 1) * 4),
                 o_words = o_koff + up16(((size_t) nb_max + 1) * 4), total = o_words + sizeof(Words);
    ecal_devbuf scratch;
    int rc;
    if ((rc = ecal_ensure(ctx, scratch, total))) return rc;
    uint8_t *base = scratch.as<uint8_t>();
    unsigned long long *first = (unsigned long long *) (base + o_first);
    uint32_t *keep = (uint32_t *) (base + o_keep), *koff = (uint32_t *) (base + o_koff);
    Words *d_w = (Words *) (base + o_words);
    if ((rc = ecal_ingest_wipe_words(ctx, d_w, sizeof(Words), &d_w->first_stop, st))) return rc;
    tm.mark("start");
    src.first = first;
    src.n_slots = bound;
    uint32_t nb = nb_max;
    launch_scan(first, d_w);
    ECAL_HIP_TRY(ctx, hipGetLastError());
    tm.mark(N.scan_mark);
    if (n_slots_host == NONE) {   // the grid is a count of the table: one look at it
        Words W;
        if ((rc = ecal_ingest_fetch_words(ctx, &W, d_w, sizeof(W), st))) return rc;
        if (W.bad_table) {
            ctx->last_error = who + ": " + std::to_string(W.bad_table) + " " + entry + "s of the table do not lie within the " + holder;
            return ECAL_ERR_INVALID;
        }
        if (W.n_slots > 0xFFFFFFFFull) {
            I.n_events = W.n_slots;
            ctx->last_error = who + ": more than 2^32-1 events";
            return ECAL_ERR_RANGE;
        }
        if (W.n_slots > bound) {   // (entries that overlap: more events than the file has room for)
            ctx->last_error = who + ": the " + entry + " table names more events than the " + holder + " holds";
            return ECAL_ERR_INVALID;
        }
        src.n_slots = W.n_slots;
        nb = (uint32_t) ((W.n_slots + block_events - 1) / block_events);
    }
    I.n_raw_events = src.n_slots;
    if (!src.n_slots) return ECAL_OK;
    if (own_events) {
        capacity = src.n_slots;
        if ((rc = ecal_ingest_alloc_records(ctx, N.who, capacity, own_events))) return rc;
        d_events = *own_events;
    }
    return ecal_ingest_verdict_write(
        ctx, N.who, tm, nb, keep, koff, (const Words *) d_w, capacity, own_events, I, st, [&] { launch_verdict(src, flt, nb, keep, d_w); },
        [&] { launch_write(src, flt, nb, (const uint32_t *) koff, d_events, capacity, d_w); },
        [&](const Words &W, uint64_t *n_more) -> int {
            if (W.bad_table || W.n_slots != src.n_slots) {
                ctx->last_error = who + ": the " + entry + " table does not fit the " + holder + " (" + std::to_string(W.bad_table) + " " + entry +
                                  "s outside it, " + std::to_string(W.n_slots) + " events)";
                return ECAL_ERR_INVALID;
            }
            return after(W, n_more);
        });
}
