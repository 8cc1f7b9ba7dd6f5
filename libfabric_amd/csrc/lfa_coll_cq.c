/*
 * lfa_coll_cq.c — the queue of in-flight operations of the collective
 * provider and its completions (liblfa_coll.so; split out of lfa_coll.c):
 * the event pool, the FIFO ring and its enqueue forms, progress (reaping in
 * issue order, coll_ep_progress, coll_coll.c:816-890), lfa_cq_read,
 * lfa_cq_readerr, lfa_eq_read and lfa_coll_ep_flush.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "lfa_coll_int.h"

LFA_INTERNAL void release_event(struct lfa_coll_ep *ep, hipEvent_t ev)
{
	if (ep->nev < (int)(sizeof(ep->evpool) / sizeof(ep->evpool[0])))
		ep->evpool[ep->nev++] = ev;
	else
		hipEventDestroy(ev);
}

/* A completion event from the endpoint's pool (ep->lock held): creating
 * one costs a runtime call per operation otherwise.  NULL on failure. */
LFA_INTERNAL hipEvent_t event_get(struct lfa_coll_ep *ep)
{
	hipEvent_t ev;

	if (ep->nev)
		return ep->evpool[--ep->nev];
	return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : NULL;
}

/* Room for `n` more operations in the FIFO of in-flight operations (the
 * ring doubles as needed): 0 or -LFA_ENOMEM. */
LFA_INTERNAL int queue_reserve(struct lfa_coll_ep *ep, size_t n)
{
	size_t cap = ep->qcap;

	while (cap - ep->qlen < n)
		cap *= 2;
	if (cap != ep->qcap) {
		struct pending *nq = calloc(cap, sizeof(*nq));

		if (!nq)
			return -LFA_ENOMEM;
		for (size_t i = 0; i < ep->qlen; i++)
			nq[i] = ep->q[(ep->qhead + i) % ep->qcap];
		free(ep->q);
		ep->q = nq;
		ep->qhead = 0;
		ep->qcap = cap;
	}
	return 0;
}

/* The free slot at the tail of the FIFO, zeroed but for the fields every
 * operation has; the caller completes it and counts it in (ep->qlen++). */
static struct pending *queue_slot(struct lfa_coll_ep *ep, void *context,
				  enum pending_kind kind, struct lfa_coll_mc *mc)
{
	struct pending *p;

	if (queue_reserve(ep, 1))
		return NULL;
	p = &ep->q[(ep->qhead + ep->qlen) % ep->qcap];
	memset(p, 0, sizeof(*p));
	p->context = context;
	p->kind = kind;
	p->mc = mc;
	return p;
}

LFA_INTERNAL struct pending *enqueue_completion(struct lfa_coll_ep *ep, hipStream_t s,
					  void *context, enum pending_kind kind,
					  struct lfa_coll_mc *mc, struct op_done done,
					  int *err)
{
	struct pending *p = queue_slot(ep, context, kind, mc);

	*err = -LFA_ENOMEM;
	if (!p)
		return NULL;
	if (done.val) {
		/* the kernel stores done.val into the completion word: no event
		 * to record or query.  p->ww stays unarmed: its bound starts at
		 * the head of the queue */
		p->done = done;
		if (ep->drop_words > 0) {
			/* test knob: a value the word never reaches */
			ep->drop_words--;
			p->done.val |= 1ull << 62;
		}
	} else {
		*err = -LFA_EIO;
		p->ev = event_get(ep);
		if (!p->ev)
			return NULL;
		if (hipEventRecord(p->ev, s) != hipSuccess) {
			release_event(ep, p->ev);
			return NULL;
		}
	}
	ep->qlen++;
	*err = 0;
	return p;
}

LFA_INTERNAL struct pending *enqueue_host(struct lfa_coll_ep *ep, struct hop *h,
				    void *context, enum pending_kind kind,
				    struct lfa_coll_mc *mc, int *err)
{
	struct pending *p = queue_slot(ep, context, kind, mc);

	*err = p ? 0 : -LFA_ENOMEM;
	if (!p)
		return NULL;
	p->hop = h;
	ep->qlen++;
	/* kick: run up to the first transfer now (coll_progress_work) */
	host_progress_all(ep);
	return p;
}

/* Completion state of a queued operation: 0 done, 1 pending, <0 / hip error
 * code (>0 in *perr) failed. */
static int pending_state(const struct lfa_coll_ep *ep, struct pending *p,
			 int *perr)
{
	if (p->hop) {
		if (p->hop->err) {
			/* the failing HIP call's code when there was one */
			*perr = p->hop->r.hip_err ? p->hop->r.hip_err : -p->hop->err;
			return -1;
		}
		return p->hop->done ? 0 : 1;
	}
	if (p->done.val) {
		const uint64_t *w = p->done.w ? p->done.w : ep->done_word;

		if (*(const volatile uint64_t *)w >= p->done.val)
			return 0;
		return word_overdue(ep, w, ep->stream, &p->ww, perr);
	}
	hipError_t e = hipEventQuery(p->ev);

	if (e == hipErrorNotReady)
		return 1;
	if (e != hipSuccess) {
		*perr = (int)e;
		return -1;
	}
	return 0;
}

/* failed: the operation was reaped in error (a word timeout, a failed queue
 * or stream) — its kernel may still run later and read or write its bounce
 * block, so the block leaves the pool for good instead of going back to be
 * refilled by the next submit (done_word_free keeps owed words
 * the same way).  A hop's own free synchronises its stream first. */
static void pending_release(struct lfa_coll_ep *ep, struct pending *p, int failed)
{
	if (p->hop)
		hop_free(p->hop);
	else if (p->ev)
		release_event(ep, p->ev);
	if (failed && !p->hop)
		bounce_retire(ep, p->bounce.block);
	else
		bounce_put(ep, p->bounce.block);
	p->hop = NULL;
	p->ev = NULL;
	p->bounce.block = NULL;
}

/* Reap completed operations in issue order. */
static void progress(struct lfa_coll_ep *ep, struct lfa_cq_entry *out,
		     size_t count, size_t *nout)
{
	*nout = 0;
	if (ep->dom->host)
		host_progress_all(ep);
	while (ep->qlen && !ep->have_err) {
		struct pending *p = &ep->q[ep->qhead];
		int perr = 0, st = pending_state(ep, p, &perr);

		if (st > 0)
			break;
		if (st == 0 && p2p_timed_out(p)) {
			/* a flag barrier or one-shot wait of this operation, or of
			 * an earlier one of its group, gave up waiting for a member
			 * (lfa_signal.h): this one and every later P2P operation of
			 * the group fail; the earlier ones completed normally */
			if (p->pmc)
				p->pmc->sig_failed = 1;
			st = -1;
			perr = ETIMEDOUT;
		} else if (st < 0 && p->pmc) {
			/* a P2P operation reaped as failed for another cause (its
			 * word's bound, a failed queue or stream): its kernel may
			 * still run and post into the workspace, so the group takes
			 * no further P2P operation and its workspace goes to the
			 * quarantine at close, as after a timed-out wait */
			p->pmc->sig_failed = 1;
		}
		if (st == 0)
			bounce_finish(&p->bounce);
		if (p->chain && p->chain == ep->failed_chain) {
			/* a chunk of an operation whose error was already
			 * reported: its outcome is that error, no second entry */
		} else if (p->kind == PEND_COLL && st == 0 && *nout >= count) {
			break;
		} else if (st < 0) {
			ep->err.op_context = p->context;
			ep->err.flags = LFA_COLLECTIVE;
			/* a word operation's own cause (ETIMEDOUT / EIO), else EIO
			 * with the HIP code as prov_errno */
			ep->err.err = p->hop || (p->done.val && (perr == ETIMEDOUT || perr == EIO))
				      ? perr : LFA_EIO;
			ep->err.prov_errno = perr;
			ep->have_err = 1;
			if (p->chain)
				ep->failed_chain = p->chain;
		} else if (p->kind == PEND_JOIN) {
			join_finish(ep, p->mc);
		} else if (p->kind == PEND_COLL) {
			struct lfa_cq_entry *c = &out[(*nout)++];

			memset(c, 0, sizeof(*c));
			c->op_context = p->context;
			c->flags = LFA_COLLECTIVE;
		}
		/* PEND_JOIN_CLOSED, PEND_CHUNK: nothing to post (a chunk's
		 * operation completes with its last chunk, peer_chunked) */
		if (st == 0 && p->done.val)
			ep->word_ops++;
		pending_release(ep, p, st < 0);
		ep->qhead = (ep->qhead + 1) % ep->qcap;
		ep->qlen--;
	}
	if (ep->stage_trim_due && !ep->qlen) {
		stage_trim(ep, ep->stage_cap);
		ep->stage_trim_due = 0;
	}
}

ssize_t lfa_cq_read(struct lfa_coll_ep *ep, struct lfa_cq_entry *buf,
		    size_t count)
{
	size_t n;
	int have_err;
	ncclResult_t async;

	if (!ep || (!buf && count))
		return -LFA_EINVAL;
	pthread_mutex_lock(&ep->lock);
	progress(ep, buf, count, &n);
	if (!n && !ep->have_err && !ep->dom->host &&
	    ncclCommGetAsyncError(ep->dom->comm, &async) == ncclSuccess &&
	    async != ncclSuccess && async != ncclInProgress) {
		ep->err.op_context = ep->qlen ? ep->q[ep->qhead].context : NULL;
		ep->err.flags = LFA_COLLECTIVE;
		ep->err.err = LFA_EIO;
		ep->err.prov_errno = (int)async;
		ep->have_err = 1;
	}
	have_err = ep->have_err;
	pthread_mutex_unlock(&ep->lock);
	if (n)
		return (ssize_t)n;
	return have_err ? -LFA_EIO : -LFA_EAGAIN;
}

ssize_t lfa_cq_readerr(struct lfa_coll_ep *ep, struct lfa_cq_err_entry *buf)
{
	ssize_t ret = -LFA_EAGAIN;

	if (!ep || !buf)
		return -LFA_EINVAL;
	pthread_mutex_lock(&ep->lock);
	if (ep->have_err) {
		*buf = ep->err;
		ep->have_err = 0;
		ret = 1;
	}
	pthread_mutex_unlock(&ep->lock);
	return ret;
}

ssize_t lfa_eq_read(struct lfa_coll_ep *ep, uint32_t *event,
		    struct lfa_eq_entry *entry)
{
	struct lfa_cq_entry tmp[1];
	size_t n;
	ssize_t ret = -LFA_EAGAIN;

	if (!ep || !event || !entry)
		return -LFA_EINVAL;
	pthread_mutex_lock(&ep->lock);
	/* progress joins only up to the first collective completion */
	while (ep->qlen && ep->q[ep->qhead].kind == PEND_JOIN && !ep->have_err) {
		int perr;

		progress(ep, tmp, 0, &n);
		if (ep->qlen && ep->q[ep->qhead].kind == PEND_JOIN &&
		    pending_state(ep, &ep->q[ep->qhead], &perr) > 0)
			break;
	}
	if (ep->dom->host && !(ep->qlen && ep->q[ep->qhead].kind == PEND_JOIN))
		host_progress_all(ep);
	if (ep->eqn) {
		*event = ep->eq[ep->eqh].event;
		*entry = ep->eq[ep->eqh].entry;
		ep->eqh = (ep->eqh + 1) % 64;
		ep->eqn--;
		ret = (ssize_t)sizeof(*entry);
	}
	pthread_mutex_unlock(&ep->lock);
	return ret;
}

int lfa_coll_ep_flush(struct lfa_coll_ep *ep)
{
	if (!ep)
		return -LFA_EINVAL;
	if (ep->dom->host) {
		/* drive the transfers until every queued operation finished */
		for (;;) {
			int busy = 0, err = 0;

			pthread_mutex_lock(&ep->lock);
			host_progress_all(ep);
			for (size_t i = 0; i < ep->qlen; i++) {
				struct hop *h = ep->q[(ep->qhead + i) % ep->qcap].hop;

				if (h && h->err)
					err = h->err;
				else if (h && !h->done)
					busy = 1;
			}
			if (!busy && !err)
				stage_trim(ep, 0);
			pthread_mutex_unlock(&ep->lock);
			if (err)
				return err;
			if (!busy)
				return 0;
			sched_yield();
		}
	}
	return hipStreamSynchronize(ep->stream) == hipSuccess &&
	       hipStreamSynchronize(ep->copy_stream) == hipSuccess &&
	       hipStreamSynchronize(ep->d2h_stream) == hipSuccess ? 0 : -LFA_EIO;
}
