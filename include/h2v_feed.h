/* h2v_feed.h — feed a launched staged batch to a resident accumulator without a host wait: an extension of the C ABI of
 * include/h2v.h, exported by the same library.
 *
 * h2v_accumulator_process_batch (h2v.h) takes the G groups of a FINISHED batch as G legs and returns with the accumulator's stream
 * idle: the caller waits for the launch first, and for the feed second.  h2v_accumulator_feed_batch is the same operation ENQUEUED:
 *     (L, R) <- (prod_g M_g) (L, R) + sum_g W_g S_g,     W_g = prod_{f > g} M_f
 * with the groups' sums S_g and the products M_g of their draws taken from what the launch leaves on the device, and it waits for
 * nothing.  A loop of upload (from device memory or from a seed), launch, feed_batch never stops the host; h2v_accumulator_settle,
 * whenever the caller wants it, waits once and brings the host's bookkeeping up to date.
 *
 * The definition.  feed_batch(b); settle equals process_batch(b) after a host finish of the same launch, which equals
 * h2v_accumulator_process once per group: the bytes and counters h2v_accumulator_read reports, h2v_accumulator_check_legs' rows and
 * what h2v_accumulator_drop_legs does afterwards, bit for bit, for any number of feeds of any number of batches in front of one
 * settle.
 *
 * Who waits for what — all of it on the device.
 *   1. On the batch's stream: whatever the last launch left on the batch's auxiliary stream is joined and the whole accumulators are
 *      made, as h2v_batch_finish_device begins.  An event is recorded there and the accumulator's stream waits for it.
 *   2. On the accumulator's stream, first everything that READS the batch: its sums, the status words (counted per group into scratch
 *      of the accumulator's own), the first draw and multiplier of every group and, after h2v_batch_upload_device, the fault word of
 *      the upload's verdict.  Kernels, no copy engine.  Then the READ EVENT, which the batch owns, is recorded.
 *   3. Behind it the scale step over G + 1 items, the fold that writes the journal slots and then (L, R) — the only write to the
 *      accumulator, as ever — and the kernel that writes the report.
 *   The batch respects the read event: every h2v_batch_* call that enqueues work makes the batch's stream wait for it before anything
 *   else, so after feed_batch returns the batch may be uploaded again AT ONCE.  An upload that must free one of the arrays a feed
 *   reads (a larger plan, more draws), h2v_batch_set_groups, h2v_batch_set_group_sizes and h2v_batch_destroy wait for the event on the
 *   host.  A batch that is never fed enqueues exactly what it did before this header existed.
 *
 * Lifetimes.  The batch must outlive the read event — h2v_batch_destroy sees to that — and nothing more: once the event has passed
 * the feed holds no address of the batch.  The accumulator must outlive its feeds: h2v_accumulator_destroy waits for its stream.  What
 * the HOST writes for a pending feed — the journal slots it reserved — and what the device writes for the host — the report — live in
 * pinned memory of that feed's own until the feed has been reported; the accumulator's device scratch is shared by its feeds, which
 * stream order serialises.  A batch bound to a caller's stream (h2v_batch_set_stream) is fed the same way.
 *
 * The report.  The last kernel of a feed writes, into mapped pinned memory, rc, n, G, the number of failing proofs and per group M_g,
 * its size and its count of non-zero statuses — counted from the device's status words, not from a host block.  settle reads it.
 *
 * Soundness.  The feed adds no draw and no pairing: the legs are process' legs, and (L, R) passes the final pairing under the same
 * bound as process_batch's.  What the host could refuse before and cannot see now is refused on the device:
 *   - a draw >= r in a tail uploaded from device memory.  The kernel that forms the weights reads the fault word; on a fault it writes
 *     prod M = 1 and every W_g = 0, so (L, R) keeps its value, and the report's rc is H2V_ERR_BAD_ARGUMENT.  At settle the slots go
 *     back, no journal entry appears, and BOTH counters grow by n: the launch's proofs count as processed and failed, so no later
 *     h2v_accumulator_finalize reports ok over a feed that was dropped.  (The caller still learns of it from rc, per feed.  After an
 *     h2v_accumulator_drop_legs the counters are those of the journal's entries, as h2v.h says: a dropped feed holds no entry and
 *     added nothing to the points, and is forgotten there like every dropped leg.)
 *   - a proof with a status: its terms are out of the sums already (the launch zeroes them); its group's failed count in the report
 *     is what keeps finalize from reporting ok, as in process_batch.
 *   A pairing-only bad proof is found as ever: the journal, h2v_accumulator_check_legs, h2v_accumulator_drop_legs.
 *   Until settle has returned the host knows nothing of a feed: counters, entries and reports describe settled feeds only.
 *
 * Every other h2v_accumulator_* call — process, process_hinted, process_guards, process_batch, add_msm, add_msms, read, finalize,
 * journal_begin, check_legs, drop_legs, merge (on the destination and on every source), merge_states, export_state, destroy —
 * settles first; the reports of feeds settled that way stay queued for the next h2v_accumulator_settle.  The invariant of h2v.h,
 * "the accumulator's stream is idle whenever a call returns", becomes "idle, or holding only enqueued feeds".
 *
 * Threading.  An accumulator and a batch are each used from one thread at a time, as in h2v.h; feed_batch uses both.  The entry
 * points are not named in the scene table that covers include/h2v.h (tests/thread_scenes.py), and join h2v.h when that table is next
 * revised.  Errors are reported as in h2v.h (h2v_last_error, per thread).
 */
#ifndef H2V_FEED_H
#define H2V_FEED_H

#include "h2v.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Feeds of one accumulator that h2v_accumulator_settle has not handed out yet; one more is H2V_ERR_UNSUPPORTED. */
#define H2V_FEED_MAX_PENDING 64

/* h2v_accumulator_process_batch, enqueued.  The batch is launched or finished; its stage does not change and the call may be repeated
 * (every call is a feed of its own).  Refused with H2V_ERR_BAD_ARGUMENT, before any device work and with both objects untouched: a
 * batch with nothing launched, a fold since the launch, a shard (n_tail != n), multipliers that are not the upload's, a guard-variant
 * upload, a batch on another device or over other params (g[0], g2, s_g2) than the accumulator, more than 512 groups.
 * H2V_ERR_UNSUPPORTED, likewise: a journal with fewer free entries than the batch has groups, the legs of the feeds still unsettled
 * counted; H2V_FEED_MAX_PENDING feeds not handed out yet.  An upload of no proofs enqueues nothing and leaves no report.
 * The call waits for nothing: no synchronise of a stream or an event, no copy. */
int h2v_accumulator_feed_batch(h2v_accumulator* a, h2v_batch* b);

/* Host state only: *n_unsettled = the feeds enqueued since the last settle of any kind, *n_unreported = the feeds whose report
 * h2v_accumulator_settle has not handed out yet (>= *n_unsettled).  Either output may be NULL. */
int h2v_accumulator_pending(const h2v_accumulator* a, size_t* n_unsettled, size_t* n_unreported);

/* Waits for the accumulator's stream, commits the host bookkeeping of every unsettled feed in feed order — the counters, and with the
 * journal on one entry per group (slot, M_g, size, failed) — and hands out the reports of ALL feeds since the last call of this
 * function, in feed order: feed_rc[i] is 0 or H2V_ERR_BAD_ARGUMENT (a draw >= r: the feed changed nothing but the counters),
 * feed_proofs[i] its n, feed_failed[i] its failing proofs (n for a dropped feed).  *n_feeds = their number.
 * cap == 0 with NULL arrays asks for the count and hands out nothing (h2v_accumulator_check_legs' convention); arrays with cap below
 * the count: H2V_ERR_BAD_ARGUMENT, and the reports are kept.  Any of the three arrays may be NULL. */
int h2v_accumulator_settle(h2v_accumulator* a, size_t cap, size_t* n_feeds, int* feed_rc, size_t* feed_proofs, size_t* feed_failed);

#ifdef __cplusplus
}
#endif

#endif
