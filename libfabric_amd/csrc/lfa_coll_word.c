/*
 * lfa_coll_word.c — completion words and direct dispatch of the collective
 * provider (liblfa_coll.so; split out of lfa_coll.c in round 6).
 *
 * Small operations complete through a host-mapped word their kernel's last
 * workgroup stores, instead of a HIP event: the word's wait
 * bound and error path, the endpoint's counter and word, the direct HSA
 * queue shared per device, and a one-member group's solo copy.  The
 * reference's completion is coll_collective_comp (coll_coll.c:722-756).
 */
#define _GNU_SOURCE
#include <dirent.h>
#include <errno.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "lfa_coll_int.h"

static uint64_t mono_ns(void)
{
	struct timespec t;

	clock_gettime(CLOCK_MONOTONIC, &t);
	return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
}

/*
 * Operations completed by a host-mapped word.  The host reads
 * the word on every poll; a word that never comes — the queue or stream owing
 * it failed, or its kernel never ran — would otherwise hold every later
 * completion of the endpoint (they are reaped in issue order).  So at most
 * every LFA_WORD_CHECK_NS a poll also asks the direct queue whether it has
 * failed, or the stream whether it reports an error, and past the deadline
 * (LFA_SIG_TIMEOUT_MS, the bound of every other GPU wait of the provider,
 * counted from the first poll that finds the operation at the head of the
 * queue: since round 6) the operation fails with ETIMEDOUT.  The failing operation
 * is reaped once, as an error entry; the word's later arrival is harmless,
 * the words only ever grow.
 */
#define LFA_WORD_CHECK_NS 1000000ull

static void word_wait_start(const struct lfa_coll_ep *ep, struct word_wait *ww)
{
	ww->checked_ns = mono_ns();
	ww->deadline_ns = ww->checked_ns + ep->word_timeout_ns;
	ww->armed = 1;
}

/* A word not yet at its value: 1 still pending, -1 failed with *perr =
 * ETIMEDOUT, EIO (the direct queue failed) or the stream's HIP error code. */
LFA_INTERNAL int word_overdue(const struct lfa_coll_ep *ep, const uint64_t *w, hipStream_t s,
			struct word_wait *ww, int *perr)
{
	uint64_t now;

	if (!ww->armed) {
		/* first poll at the head of the queue: nothing ahead of this
		 * operation is still owed, its own bound starts now */
		word_wait_start(ep, ww);
		return 1;
	}
	now = mono_ns();
	if (now - ww->checked_ns < LFA_WORD_CHECK_NS)
		return 1;
	ww->checked_ns = now;
	if (ep->direct && w == ep->ddone_word) {
		if (lfa_direct_failed(ep->direct)) {
			*perr = EIO;
			return -1;
		}
	} else if (s) {
		hipError_t e = hipStreamQuery(s);

		if (e != hipSuccess && e != hipErrorNotReady) {
			(void)hipGetLastError();
			*perr = (int)e;
			return -1;
		}
	}
	if (now >= ww->deadline_ns) {
		*perr = ETIMEDOUT;
		return -1;
	}
	return 1;
}

/* The completion word and its counter (device endpoints), zeroed. */
LFA_INTERNAL int done_word_init(struct lfa_coll_ep *ep)
{
	if (hipMalloc((void **)&ep->done_ctr, sizeof(uint32_t)) != hipSuccess) {
		ep->done_ctr = NULL;
		return -1;
	}
	if (hipHostMalloc((void **)&ep->done_word, sizeof(uint64_t),
			  hipHostMallocCoherent) != hipSuccess) {
		ep->done_word = NULL;
		return -1;
	}
	*(volatile uint64_t *)ep->done_word = 0;
	return hipMemset(ep->done_ctr, 0, sizeof(uint32_t)) == hipSuccess ? 0 : -1;
}

/*
 * One direct queue per device and process, shared by its endpoints (each
 * keeps its own counter and completion word): a hardware queue is a scarce
 * resource — past ~20 on the GPU the scheduler time-slices —
 * and the queue's packets run in order whichever endpoint wrote them.
 */
#define DIRECT_DEVS 64
static struct {
	struct lfa_direct *d;
	int refs, failed;
} shared_direct[DIRECT_DEVS];
static pthread_mutex_t direct_lock = PTHREAD_MUTEX_INITIALIZER;

static struct lfa_direct *direct_acquire(int dev)
{
	struct lfa_direct *d = NULL;

	if (dev < 0 || dev >= DIRECT_DEVS)
		return NULL;
	pthread_mutex_lock(&direct_lock);
	if (!shared_direct[dev].d && !shared_direct[dev].failed) {
		shared_direct[dev].d = lfa_direct_open(dev);
		shared_direct[dev].failed = !shared_direct[dev].d;
	}
	d = shared_direct[dev].d;
	if (d)
		shared_direct[dev].refs++;
	pthread_mutex_unlock(&direct_lock);
	return d;
}

static void direct_release(int dev)
{
	pthread_mutex_lock(&direct_lock);
	if (shared_direct[dev].d && --shared_direct[dev].refs == 0) {
		lfa_direct_close(shared_direct[dev].d);
		shared_direct[dev].d = NULL;
	}
	pthread_mutex_unlock(&direct_lock);
}

/*
 * `stream_ok`: the endpoint's streams drained (lfa_coll_ep_flush), so no
 * kernel on them still writes done_ctr / done_word.  The direct queue's
 * kernels are on no stream: its last word is awaited (bounded).  A counter
 * or word that a packet still queued may write is never freed:
 * it is left allocated, with the queue reference that keeps the queue alive,
 * and the leak is reported on stderr.
 */
LFA_INTERNAL void done_word_free(struct lfa_coll_ep *ep, int stream_ok)
{
	if (ep->direct) {
		const uint64_t t0 = mono_ns();

		/* a failed queue's kernels may still finish (a test marks a
		 * working queue failed): a short grace, else the full bound */
		while (*(volatile uint64_t *)ep->ddone_word < ep->ddone_seq &&
		       mono_ns() - t0 < (lfa_direct_failed(ep->direct) ? 100000000ull
								 : ep->word_timeout_ns))
			sched_yield();
		if (*(volatile uint64_t *)ep->ddone_word < ep->ddone_seq) {
			fprintf(stderr, "lfa: endpoint closed with direct-queue word %llu of %llu: "
				"its counter, word and queue are left allocated\n",
				(unsigned long long)*(volatile uint64_t *)ep->ddone_word,
				(unsigned long long)ep->ddone_seq);
			ep->ddone_ctr = NULL;
			ep->ddone_word = NULL;
		} else {
			direct_release(ep->dom->device);
		}
		ep->direct = NULL;
	}
	if (!stream_ok && ep->done_word) {
		fprintf(stderr, "lfa: endpoint closed with its stream not drained: its "
			"completion counter and word are left allocated\n");
		ep->done_ctr = NULL;
		ep->done_word = NULL;
	}
	if (ep->ddone_ctr)
		hipFree(ep->ddone_ctr);
	if (ep->ddone_word)
		hipHostFree(ep->ddone_word);
	ep->ddone_ctr = NULL;
	ep->ddone_word = NULL;
	if (ep->done_ctr)
		hipFree(ep->done_ctr);
	if (ep->done_word)
		hipHostFree(ep->done_word);
	ep->done_ctr = NULL;
	ep->done_word = NULL;
}

int lfa_coll_ep_test_word(struct lfa_coll_ep *ep, int drop_next, long timeout_ms,
			  int fail_direct)
{
	if (!ep || drop_next < 0)
		return -LFA_EINVAL;
	pthread_mutex_lock(&ep->lock);
	ep->drop_words = drop_next;
	if (timeout_ms > 0)
		ep->word_timeout_ns = (uint64_t)timeout_ms * 1000000ull;
	if (fail_direct && ep->direct)
		lfa__direct_mark_failed(ep->direct);
	pthread_mutex_unlock(&ep->lock);
	return 0;
}

uint64_t lfa_coll_ep_word_ops(struct lfa_coll_ep *ep)
{
	uint64_t n;

	if (!ep)
		return 0;
	pthread_mutex_lock(&ep->lock);
	n = ep->word_ops;
	pthread_mutex_unlock(&ep->lock);
	return n;
}

int lfa_coll_ep_test_solo(struct lfa_coll_ep *ep, size_t max_bytes)
{
	if (!ep || max_bytes > ((size_t)1 << 30))
		return -LFA_EINVAL;
	pthread_mutex_lock(&ep->lock);
	ep->solo_max = max_bytes;
	pthread_mutex_unlock(&ep->lock);
	return 0;
}

int lfa_coll_ep_uses_direct(struct lfa_coll_ep *ep)
{
	if (!ep)
		return -LFA_EINVAL;
	return ep->direct ? (lfa_direct_failed(ep->direct) ? 2 : 1) : 0;
}

/*
 * A small reducing collective of a one-member group (allreduce, reduce,
 * reduce_scatter: each a copy of the input) as one launch that ends in the
 * completion word, so the operation completes without an event (VERDICT r3
 * #4; the plan would be one COPY item plus an event record and query).
 */
/* The direct queue for this endpoint's device, opened at first use. */
static struct lfa_direct *direct_of(struct lfa_coll_ep *ep)
{
	const char *e;

	if (ep->direct || ep->direct_tried)
		return ep->direct;
	ep->direct_tried = 1;
	e = lfa_param("LFA_DIRECT");
	if (e && e[0] == '0')
		return NULL;
	if (hipMalloc((void **)&ep->ddone_ctr, sizeof(uint32_t)) != hipSuccess ||
	    hipMemset(ep->ddone_ctr, 0, sizeof(uint32_t)) != hipSuccess ||
	    hipHostMalloc((void **)&ep->ddone_word, sizeof(uint64_t),
			  hipHostMallocCoherent) != hipSuccess) {
		(void)hipGetLastError();
		return NULL;
	}
	*(volatile uint64_t *)ep->ddone_word = 0;
	ep->direct = direct_acquire(ep->dom->device);
	return ep->direct;
}

/* The largest world-1 reducing collective run_solo takes: LFA_ONESHOT_SOLO_BYTES
 * unless LFA_SOLO_BYTES says otherwise (a tuning knob). */
LFA_INTERNAL size_t solo_bytes(void)
{
	static long long v = -1;

	if (v < 0) {
		const char *e = lfa_param("LFA_SOLO_BYTES");
		const long long x = e ? atoll(e) : -1;

		v = x >= 0 && x <= (1ll << 30) ? x : (long long)LFA_ONESHOT_SOLO_BYTES;
	}
	return (size_t)v;
}

LFA_INTERNAL int run_solo(struct lfa_coll_ep *ep, const void *buf, void *result, size_t count,
		    enum lfa_datatype dt, int direct, struct op_done *done)
{
	int ret;

	if (direct && count * lfa_reduce_datatype_size(dt) <= LFA_DIRECT_SOLO_BYTES &&
	    direct_of(ep) && !lfa_direct_failed(ep->direct)) {
		/* no HIP launch: ~3 us less host time */
		ret = lfa_direct_solo_copy(ep->direct, result, buf, count * lfa_reduce_datatype_size(dt),
					   ep->ddone_ctr, ep->ddone_word, ep->ddone_seq + 1);
		if (!ret) {
			*done = (struct op_done){ ++ep->ddone_seq, ep->ddone_word };
			return 0;
		}
		if (ret != -LFA_EIO)
			return ret;
		/* the queue failed (nothing was enqueued): the HIP launch below;
		 * the operations it still owes fail in word_overdue */
	}

	/* the one-shot kernel with n = 1 gives the same bytes; this kernel's
	 * arguments are 48 bytes instead of ~700, about 1 us less from launch
	 * to the word (tools/probe_solo_latency.py) */
	ret = lfa_solo_copy_async(result, buf, count * lfa_reduce_datatype_size(dt), ep->done_ctr,
				  ep->done_word, ep->done_seq + 1, ep->stream);
	if (ret)
		return ret;
	*done = (struct op_done){ ++ep->done_seq, NULL };
	return 0;
}
