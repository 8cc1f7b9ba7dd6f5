/*
 * lfa_coll_plan.c — the schedule builder of the collective provider: a
 * collective becomes an array of lfa_step items for one rank (lfa_coll_plan,
 * include/lfa_coll.h), host-only and testable on CPU.  prov/coll builds the
 * same thing as a work queue per operation (include/ofi_coll.h:64-119,
 * coll_coll.c:229-343); the executor that runs these schedules over RCCL or
 * the owner's transfers is lfa_coll_exec.c.
 *
 * Everything is emitted through ONE planner (push and the p_* helpers below):
 * the algorithms, and lower_plan's rewriting of a finished plan.  The planner
 * owns its arrays and the one TMP total; tools/plan_host_check.c pins every
 * schedule bit for bit (tests/test_plan_host_cpu.py).
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "lfa_atomic.h"
#include "lfa_coll.h"
#include "lfa_coll_plan.h"
#include "lfa_signal.h"

void lfa_coll_block(size_t count, int nranks, int r, size_t *off, size_t *len)
{
	size_t base = count / (size_t)nranks, extra = count % (size_t)nranks;
	size_t rr = (size_t)r;

	*len = base + (rr < extra ? 1 : 0);
	*off = rr * base + (rr < extra ? rr : extra);
}

void lfa_coll_io_bytes(enum lfa_collective_op coll, size_t count, int nranks,
		       int rank, int root, size_t esz, size_t *in_bytes,
		       size_t *out_bytes)
{
	size_t off, len;

	*in_bytes = *out_bytes = count * esz;
	switch (coll) {
	case LFA_REDUCE_SCATTER:
		lfa_coll_block(count, nranks, rank, &off, &len);
		*out_bytes = len * esz;
		break;
	case LFA_REDUCE:
		if (rank != root)
			*out_bytes = 0;
		break;
	case LFA_ALLGATHER:
		*out_bytes = (size_t)nranks * count * esz;
		break;
	case LFA_SCATTER:
		*in_bytes = rank == root ? (size_t)nranks * count * esz : 0;
		break;
	default:
		break;
	}
}

/* ====================================================================== */
/* the planner: growable steps and refs, one TMP total                     */
/* ====================================================================== */

struct planner {
	struct lfa_step *steps;
	size_t cap, n;
	struct lfa_ref *refs;
	size_t rcap, nr;
	int pending_comm;       /* SEND/RECV since the last GROUP_END */
	int nomem;              /* an array could not grow: the plan is void */
	uint64_t tmp;           /* TMP bytes laid out so far (p_tmp) */
	struct lfa_step sink;   /* where items go once nomem is set */
};

/* What is planned: one rank's view of one collective. */
struct job {
	enum lfa_collective_op coll;
	int r, n, root;
	size_t count, esz;
	size_t bytes;           /* count·esz */
	size_t moff, mlen;      /* rank r's block of count (lfa_coll_block) */
};

/* `arr`, grown to hold item n; NULL (and nomem) when it cannot.  It starts
 * small: peer domains plan every operation, and a one-item plan should cost
 * the allocator no more than its one item. */
static void *grown(struct planner *p, void *arr, size_t *cap, size_t n, size_t size)
{
	size_t want = *cap ? 2 * *cap : 8;

	if (n < *cap)
		return arr;
	arr = p->nomem ? NULL : realloc(arr, want * size);
	if (arr)
		*cap = want;
	else
		p->nomem = 1;
	return arr;
}

/* Both arrays exist from the start, so an empty plan has them too. */
static void p_init(struct planner *p)
{
	memset(p, 0, sizeof(*p));
	p->steps = grown(p, NULL, &p->cap, 0, sizeof(*p->steps));
	p->refs = grown(p, NULL, &p->rcap, 0, sizeof(*p->refs));
}

static void p_free(struct planner *p)
{
	free(p->steps);
	free(p->refs);
}

static struct lfa_ref ref(int buf, uint64_t off)
{
	struct lfa_ref r;

	r.buf = buf;
	r.rank = 0;
	r.off = off;
	return r;
}

/* A ref into group rank `rank`'s symmetric workspace (LFA_ALGO_P2P). */
static struct lfa_ref sref(int buf, int rank, uint64_t off)
{
	struct lfa_ref r = ref(buf, off);

	r.rank = (uint32_t)rank;
	return r;
}

static struct lfa_ref ref_at(struct lfa_ref r, uint64_t off)
{
	r.off += off;
	return r;
}

static struct lfa_step *push(struct planner *p, int type)
{
	struct lfa_step *s = grown(p, p->steps, &p->cap, p->n, sizeof(*p->steps));

	if (s) {
		p->steps = s;
		s = &p->steps[p->n++];
	} else {
		s = &p->sink;
	}
	memset(s, 0, sizeof(*s));
	s->type = type;
	return s;
}

static void p_ref(struct planner *p, struct lfa_ref r)
{
	struct lfa_ref *a = grown(p, p->refs, &p->rcap, p->nr, sizeof(*p->refs));

	if (!a)
		return;
	p->refs = a;
	p->refs[p->nr++] = r;
}

/* `bytes` of TMP, starting at a multiple of `align`: the one place TMP grows,
 * called where the refs into the area are made. */
static uint64_t p_tmp(struct planner *p, uint64_t bytes, uint64_t align)
{
	uint64_t base = (p->tmp + align - 1) & ~(align - 1);

	p->tmp = base + bytes;
	return base;
}

/* A SEND or RECV as it stands (zero bytes too: the lowered barrier). */
static void p_msg(struct planner *p, int type, int peer, struct lfa_ref r,
		  uint64_t bytes)
{
	struct lfa_step *s = push(p, type);

	s->peer = peer;
	s->count = bytes;
	if (type == LFA_STEP_SEND)
		s->src = r;
	else
		s->dst = r;
	p->pending_comm = 1;
}

/* A transfer of a schedule: nothing for no bytes. */
static void p_xfer(struct planner *p, int type, int peer, struct lfa_ref r,
		   uint64_t bytes)
{
	if (bytes)
		p_msg(p, type, peer, r, bytes);
}

static void p_group_end(struct planner *p)
{
	if (!p->pending_comm)
		return;
	push(p, LFA_STEP_GROUP_END);
	p->pending_comm = 0;
}

/* The items with a dst, a src and a count: REDUCE (elements), COPY and the
 * collective transport items (bytes).  Nothing for a zero count. */
static void p_item(struct planner *p, int type, struct lfa_ref dst,
		   struct lfa_ref src, uint64_t count)
{
	struct lfa_step *s;

	p_group_end(p);
	if (!count)
		return;
	s = push(p, type);
	s->dst = dst;
	s->src = src;
	s->count = count;
}

static void p_copy(struct planner *p, struct lfa_ref dst, struct lfa_ref src,
		   uint64_t bytes)
{
	if (dst.buf == src.buf && dst.off == src.off)
		bytes = 0;      /* the same place */
	p_item(p, LFA_STEP_COPY, dst, src, bytes);
}

/* TREE / TREE_PUT over refs pushed with p_ref() since p_tree_begin(): nsrc
 * inputs, then (TREE_PUT) the extra destinations.  A zero count drops the
 * item; its refs stay. */
static uint32_t p_tree_begin(struct planner *p)
{
	p_group_end(p);
	return (uint32_t)p->nr;
}

static void p_tree_end(struct planner *p, int type, uint32_t first, uint32_t nsrc,
		       struct lfa_ref dst, uint64_t count)
{
	struct lfa_step *s;

	if (!count)
		return;
	s = push(p, type);
	s->dst = dst;
	s->first = first;
	s->nsrc = nsrc;
	if (type == LFA_STEP_TREE_PUT)
		s->peer = (int32_t)(p->nr - first - nsrc);
	s->count = count;
}

static void p_oneshot(struct planner *p, int mode, int n, uint64_t count)
{
	struct lfa_step *s;

	p_group_end(p);
	if (!count)
		return;
	s = push(p, LFA_STEP_ONESHOT);
	s->dst = ref(LFA_BUF_RESULT, 0);
	s->src = ref(LFA_BUF_SEND, 0);
	s->peer = mode;
	s->nsrc = (uint32_t)n;
	s->count = count;
}

static void p_barrier(struct planner *p)
{
	p_group_end(p);
	push(p, LFA_STEP_BARRIER);
}

/*
 * The pairwise exchange, one group: for k = 1 … n-1 send to rank r+k and
 * receive from rank r-k, which spreads the peers over the xGMI links.  A side
 * says where peer k's bytes are: `bytes` at at + k·stride, or, with esz set,
 * block k of `count` elements (lfa_coll_block) from `at`.  `emit` is p_xfer,
 * or p_msg for messages that go out empty.
 */
struct side {
	struct lfa_ref at;
	uint64_t stride, bytes;
	size_t count, esz;
};

static struct side fixed(struct lfa_ref at, uint64_t bytes)
{
	struct side s = { at, 0, bytes, 0, 0 };

	return s;
}

static struct side slots(struct lfa_ref at, uint64_t stride, uint64_t bytes)
{
	struct side s = { at, stride, bytes, 0, 0 };

	return s;
}

static struct side blocks(struct lfa_ref at, size_t count, size_t esz)
{
	struct side s = { at, 0, 0, count, esz };

	return s;
}

typedef void emit_fn(struct planner *p, int type, int peer, struct lfa_ref r,
		     uint64_t bytes);

static void emit_side(struct planner *p, emit_fn *emit, int type,
		      const struct side *s, int n, int peer)
{
	size_t off, len;

	if (s->esz) {
		lfa_coll_block(s->count, n, peer, &off, &len);
		emit(p, type, peer, ref_at(s->at, off * s->esz), len * s->esz);
	} else {
		emit(p, type, peer, ref_at(s->at, (uint64_t)peer * s->stride), s->bytes);
	}
}

static void p_ring(struct planner *p, emit_fn *emit, int r, int n,
		   struct side snd, struct side rcv)
{
	for (int k = 1; k < n; k++) {
		emit_side(p, emit, LFA_STEP_SEND, &snd, n, (r + k) % n);
		emit_side(p, emit, LFA_STEP_RECV, &rcv, n, (r - k + n) % n);
	}
	p_group_end(p);
}

static uint64_t pof2_floor(uint64_t v)
{
	uint64_t q = 1;

	while (q * 2 <= v)
		q *= 2;
	return q;
}

/* ====================================================================== */
/* LFA_ALGO_TREE                                                           */
/* ====================================================================== */

/*
 * A tree over n inputs of any size.  Up to LFA_TREE_MAX inputs it is ONE
 * TREE item (one fused kernel).  Above that it is split into whole subtrees
 * of prov/coll's recursive-doubling tree, so the bits do not change:
 * virtual rank v < pof2 is the leaf pair (in[2v+1] OP in[2v]) for v < rem
 * and in[v + rem] otherwise (coll_coll.c:366-389); aligned runs of 16
 * virtual ranks are subtrees of at most 32 inputs, each reduced into a TMP
 * partial, and the pof2/16 partials are combined by the same rule
 * (recursively, for groups above 512 ranks).  A run with k < 16 pairs is
 * the kernel's own tree for 16 + k inputs (pairs first, as in the kernel); a
 * run of 16 pairs is its plain 32-input tree, whose first level is exactly
 * the pairs.
 */
struct tree_in {
	int own;                /* input `own` is own_ref (-1: none); the rest */
	struct lfa_ref own_ref;
	uint64_t base, stride;  /* are TMP slots: input k at base + k·stride */
};

static struct lfa_ref tree_in_ref(const struct tree_in *t, int k)
{
	if (k == t->own)
		return t->own_ref;
	return ref(LFA_BUF_TMP, t->base + (uint64_t)k * t->stride);
}

#define LFA_TREE_GROUP 16       /* virtual ranks per split subtree */

static void p_tree_run(struct planner *p, const struct tree_in *in, uint64_t lo,
		       uint64_t hi, struct lfa_ref dst, uint64_t count)
{
	uint32_t first = p_tree_begin(p);

	for (uint64_t k = lo; k < hi; k++)
		p_ref(p, tree_in_ref(in, (int)k));
	p_tree_end(p, LFA_STEP_TREE, first, (uint32_t)(hi - lo), dst, count);
}

static void p_tree_any(struct planner *p, const struct tree_in *in, int n,
		       struct lfa_ref dst, uint64_t count, size_t esz)
{
	uint64_t pof2 = pof2_floor((uint64_t)n), rem = (uint64_t)n - pof2;
	struct tree_in parts;
	uint64_t ngrp;

	if (n <= LFA_TREE_MAX) {
		p_tree_run(p, in, 0, (uint64_t)n, dst, count);
		return;
	}
	ngrp = pof2 / LFA_TREE_GROUP;
	parts.own = -1;
	parts.stride = ((uint64_t)count * esz + 255) & ~(uint64_t)255;
	parts.base = p_tmp(p, ngrp * parts.stride, 256);
	for (uint64_t g = 0; g < ngrp; g++) {
		uint64_t v0 = g * LFA_TREE_GROUP, v1 = v0 + LFA_TREE_GROUP;

		p_tree_run(p, in, v0 < rem ? 2 * v0 : v0 + rem,
			   v1 < rem ? 2 * v1 : v1 + rem, tree_in_ref(&parts, (int)g),
			   count);
	}
	p_tree_any(p, &parts, (int)ngrp, dst, count, esz);
}

/*
 * Distance between the gathered blocks in TMP.  The tree kernel reads all N
 * blocks at the same offset at once; blocks exactly B apart put those N
 * streams on the same HBM channels, and the 8 x 32 MiB tree drops from
 * 71 % to 68 % of peak.  Skewing block k by k x 6 KiB lifts it to 73 %
 * (bench.py --tune-tree-layout, profiles/r01_tune_tree_layout.log).  Small
 * blocks keep the dense layout.
 */
#define LFA_TREE_SKEW_MIN (1u << 20)
#define LFA_TREE_SKEW 6144u

static uint64_t blk_stride(size_t mlen, size_t esz)
{
	uint64_t b = (uint64_t)mlen * esz;

	if (b < LFA_TREE_SKEW_MIN)
		return b;
	return ((b + 255) & ~(uint64_t)255) + LFA_TREE_SKEW;
}

/*
 * Phase 1: rank r collects block r of every rank's input.  TMP slot q
 * (block-r sized, blk_stride apart) receives rank q's block; rank r's own
 * block is read in place from SEND, its slot stays free.  Returns the tree's
 * inputs.
 */
static struct tree_in plan_gather_blocks(struct planner *p, const struct job *j)
{
	struct tree_in in;

	in.own = j->r;
	in.own_ref = ref(LFA_BUF_SEND, j->moff * j->esz);
	in.stride = blk_stride(j->mlen, j->esz);
	in.base = p_tmp(p, j->n > 1 ? (uint64_t)j->n * in.stride : 0, 1);
	p_ring(p, p_xfer, j->r, j->n, blocks(ref(LFA_BUF_SEND, 0), j->count, j->esz),
	       slots(ref(LFA_BUF_TMP, in.base), in.stride, j->mlen * j->esz));
	return in;
}

/* Phase 3: every rank's reduced block, in RESULT, to every other rank. */
static void plan_allgather_blocks(struct planner *p, const struct job *j)
{
	p_ring(p, p_xfer, j->r, j->n,
	       fixed(ref(LFA_BUF_RESULT, j->moff * j->esz), j->mlen * j->esz),
	       blocks(ref(LFA_BUF_RESULT, 0), j->count, j->esz));
}

/* Small messages: everyone gets everyone's full input, one tree per rank.
 * One exchange phase instead of two; TMP holds N full inputs. */
static void plan_allreduce_small(struct planner *p, const struct job *j)
{
	struct tree_in in;

	in.own = j->r;
	in.own_ref = ref(LFA_BUF_SEND, 0);
	in.stride = j->bytes;
	in.base = p_tmp(p, (uint64_t)j->n * j->bytes, 1);
	p_ring(p, p_xfer, j->r, j->n, fixed(ref(LFA_BUF_SEND, 0), j->bytes),
	       slots(ref(LFA_BUF_TMP, in.base), in.stride, j->bytes));
	p_tree_any(p, &in, j->n, ref(LFA_BUF_RESULT, 0), j->count, j->esz);
}

/* The default schedules; the pure transports (allgather, broadcast, scatter)
 * are the same under every algorithm. */
static int plan_tree(struct planner *p, const struct job *j)
{
	const int r = j->r, n = j->n, root = j->root;
	const size_t esz = j->esz, bytes = j->bytes;
	struct lfa_ref own = ref(LFA_BUF_RESULT, j->moff * esz);
	struct tree_in in;
	struct side res;

	switch (j->coll) {
	case LFA_ALLREDUCE:
		if (n > 1 && bytes * (size_t)n <= LFA_SMALL_AG_BYTES) {
			plan_allreduce_small(p, j);
			break;
		}
		in = plan_gather_blocks(p, j);
		p_tree_any(p, &in, n, own, j->mlen, esz);
		plan_allgather_blocks(p, j);
		break;
	case LFA_REDUCE_SCATTER:
		in = plan_gather_blocks(p, j);
		p_tree_any(p, &in, n, ref(LFA_BUF_RESULT, 0), j->mlen, esz);
		break;
	case LFA_REDUCE:
		in = plan_gather_blocks(p, j);
		if (r != root) {
			/* the block lands in this rank's own, unused TMP slot */
			own = ref(LFA_BUF_TMP, in.base + (uint64_t)r * in.stride);
			p_tree_any(p, &in, n, own, j->mlen, esz);
			p_xfer(p, LFA_STEP_SEND, root, own, j->mlen * esz);
			break;
		}
		p_tree_any(p, &in, n, own, j->mlen, esz);
		res = blocks(ref(LFA_BUF_RESULT, 0), j->count, esz);
		for (int k = 0; k < n; k++)
			if (k != root)
				emit_side(p, p_xfer, LFA_STEP_RECV, &res, n, k);
		break;
	case LFA_ALLGATHER:
		p_ring(p, p_xfer, r, n, fixed(ref(LFA_BUF_SEND, 0), bytes),
		       slots(ref(LFA_BUF_RESULT, 0), bytes, bytes));
		p_copy(p, ref(LFA_BUF_RESULT, (uint64_t)r * bytes), ref(LFA_BUF_SEND, 0),
		       bytes);
		break;
	case LFA_BROADCAST:
		/* buf is in/out: the executor binds SEND and RESULT to it */
		if (r == root) {
			for (int k = 1; k < n; k++)
				p_xfer(p, LFA_STEP_SEND, (root + k) % n,
				       ref(LFA_BUF_RESULT, 0), bytes);
		} else {
			p_xfer(p, LFA_STEP_RECV, root, ref(LFA_BUF_RESULT, 0), bytes);
		}
		break;
	case LFA_SCATTER:
		/* root's buf holds n blocks of `count`; everyone gets block r */
		if (r == root) {
			for (int k = 1; k < n; k++) {
				int to = (root + k) % n;

				p_xfer(p, LFA_STEP_SEND, to,
				       ref(LFA_BUF_SEND, (uint64_t)to * bytes), bytes);
			}
			p_copy(p, ref(LFA_BUF_RESULT, 0),
			       ref(LFA_BUF_SEND, (uint64_t)r * bytes), bytes);
		} else {
			p_xfer(p, LFA_STEP_RECV, root, ref(LFA_BUF_RESULT, 0), bytes);
		}
		break;
	default:
		return -LFA_ENOSYS;
	}
	p_group_end(p);
	return 1;
}

/* ====================================================================== */
/* LFA_ALGO_RD                                                             */
/* ====================================================================== */

/*
 * The reference's recursive-doubling schedule, item for item
 * (coll_do_allreduce, coll_coll.c:349-449), into `res` with `tmp` scratch.
 */
static void plan_rd_allreduce(struct planner *p, uint64_t local, uint64_t n,
			      size_t count, size_t esz, struct lfa_ref res,
			      struct lfa_ref tmp)
{
	uint64_t pof2 = pof2_floor(n), rem = n - pof2, newid, mask;
	uint64_t bytes = (uint64_t)count * esz;

	p_copy(p, res, ref(LFA_BUF_SEND, 0), bytes);        /* :364 memcpy */
	if (local < 2 * rem) {
		if (local % 2 == 0) {
			p_xfer(p, LFA_STEP_SEND, (int)local + 1, res, bytes);
			p_group_end(p);
			newid = (uint64_t)-1;
		} else {
			p_xfer(p, LFA_STEP_RECV, (int)local - 1, tmp, bytes);
			/* result = result OP tmp */
			p_item(p, LFA_STEP_REDUCE, res, tmp, count);
			newid = local / 2;
		}
	} else {
		newid = local - rem;
	}
	if (newid != (uint64_t)-1) {
		for (mask = 1; mask < pof2; mask <<= 1) {
			uint64_t nr = newid ^ mask;
			uint64_t remote = nr < rem ? nr * 2 + 1 : nr + rem;

			p_xfer(p, LFA_STEP_RECV, (int)remote, tmp, bytes);
			p_xfer(p, LFA_STEP_SEND, (int)remote, res, bytes);
			if (remote < local) {
				p_item(p, LFA_STEP_REDUCE, res, tmp, count);
			} else {
				p_item(p, LFA_STEP_REDUCE, tmp, res, count);
				p_copy(p, res, tmp, bytes);
			}
		}
	}
	if (local < 2 * rem) {
		if (local % 2)
			p_xfer(p, LFA_STEP_SEND, (int)local - 1, res, bytes);
		else
			p_xfer(p, LFA_STEP_RECV, (int)local + 1, res, bytes);
		p_group_end(p);
	}
}

/* Allreduce runs in RESULT with one input of TMP scratch; reduce and
 * reduce_scatter run it in TMP (scratch, then the result) and copy out. */
static int plan_rd(struct planner *p, const struct job *j)
{
	struct lfa_ref tmp, res;

	if (!coll_reduces(j->coll))
		return 0;
	if (j->coll == LFA_ALLREDUCE) {
		tmp = ref(LFA_BUF_TMP, p_tmp(p, j->n > 1 ? j->bytes : 0, 1));
		res = ref(LFA_BUF_RESULT, 0);
	} else {
		tmp = ref(LFA_BUF_TMP, p_tmp(p, j->bytes, 1));
		res = ref(LFA_BUF_TMP, p_tmp(p, j->bytes, 1));
	}
	plan_rd_allreduce(p, (uint64_t)j->r, (uint64_t)j->n, j->count, j->esz, res, tmp);
	if (j->coll == LFA_REDUCE_SCATTER)
		p_copy(p, ref(LFA_BUF_RESULT, 0), ref_at(res, j->moff * j->esz),
		       j->mlen * j->esz);
	else if (j->coll == LFA_REDUCE && j->r == j->root)
		p_copy(p, ref(LFA_BUF_RESULT, 0), res, j->bytes);
	return 1;
}

/* ====================================================================== */
/* LFA_ALGO_TREE_COLL                                                      */
/* ====================================================================== */

/* LFA_ALGO_TREE with the transport done by collective items, where the
 * blocks are even: n TMP slots filled by one item, the tree over the slots
 * in rank order — the grouped-send form's bits. */
static int plan_tree_coll(struct planner *p, const struct job *j)
{
	const int n = j->n;
	const size_t esz = j->esz, blk = j->mlen * esz;
	struct tree_in in;

	if (n > LFA_TREE_MAX)
		return 0;
	in.own = -1;
	if (j->coll == LFA_ALLREDUCE && j->bytes * (size_t)n <= LFA_SMALL_AG_BYTES) {
		/* small: every rank's whole input through ONE RCCL allgather
		 * (TMP slot k <- rank k) */
		if (n == 1)
			return 0;
		in.stride = j->bytes;
		in.base = p_tmp(p, (uint64_t)n * j->bytes, 1);
		p_item(p, LFA_STEP_ALLGATHER, ref(LFA_BUF_TMP, in.base),
		       ref(LFA_BUF_SEND, 0), j->bytes);
		p_tree_any(p, &in, n, ref(LFA_BUF_RESULT, 0), j->count, esz);
		return 1;
	}
	if (j->count % (size_t)n ||
	    (j->coll != LFA_ALLREDUCE && j->coll != LFA_REDUCE_SCATTER))
		return 0;
	/* TMP slot q <- block r of rank q (own block too) */
	in.stride = blk;
	in.base = p_tmp(p, (uint64_t)n * blk, 1);
	p_item(p, LFA_STEP_ALLTOALL, ref(LFA_BUF_TMP, in.base), ref(LFA_BUF_SEND, 0), blk);
	if (j->coll == LFA_REDUCE_SCATTER) {
		p_tree_any(p, &in, n, ref(LFA_BUF_RESULT, 0), j->mlen, esz);
		return 1;
	}
	p_tree_any(p, &in, n, ref(LFA_BUF_RESULT, j->moff * esz), j->mlen, esz);
	p_item(p, LFA_STEP_ALLGATHER, ref(LFA_BUF_RESULT, 0),
	       ref(LFA_BUF_RESULT, j->moff * esz), blk);
	return 1;
}

/* ====================================================================== */
/* LFA_ALGO_P2P                                                            */
/* ====================================================================== */

/* A byte bound from the parameter `name`, read once: 1 … 1 GiB, else dflt. */
static size_t bounded_param(long long *v, const char *name, size_t dflt)
{
	if (*v < 0) {
		const char *e = lfa_param(name);
		const long long x = e ? atoll(e) : 0;

		*v = x > 0 && x <= (1ll << 30) ? x : (long long)dflt;
	}
	return (size_t)*v;
}

size_t lfa_os_ag_bytes(void)
{
	static long long v = -1;

	return bounded_param(&v, "LFA_OS_AG_BYTES", LFA_OS_AG_BYTES_DEFAULT);
}

size_t lfa_os_rs_bytes(void)
{
	static long long v = -1;

	return bounded_param(&v, "LFA_OS_RS_BYTES", LFA_OS_RS_BYTES);
}

/* One kernel does it: push into the peers' slots, flags, tree. */
static int oneshot_fits(const struct job *j)
{
	if (j->n > LFA_OS_MAX_RANKS)
		return 0;
	return j->coll == LFA_REDUCE_SCATTER ? j->bytes <= lfa_os_rs_bytes() :
	       j->bytes * (size_t)j->n <= lfa_os_ag_bytes();
}

/*
 * Every rank stages its whole input in its own SYM_IN region (ONE copy: block
 * r itself is read in place from SEND, but copying it too, 1/n more local
 * bytes, saves the second launch the two ranges around it would need), then,
 * after a barrier, reduces its part of all inputs straight out of the peers'
 * SYM_IN over xGMI.  A closing barrier guarantees no peer still reads or
 * writes this rank's workspace once its operation completes (so the next
 * operation may overwrite it, and close may free it).
 */
static void p2p_stage_input(struct planner *p, const struct job *j)
{
	p_copy(p, sref(LFA_BUF_SYM_IN, j->r, 0), ref(LFA_BUF_SEND, 0), j->bytes);
	p_barrier(p);
}

/* Tree of elements [off, off + len) over all ranks' inputs; result to dst,
 * and with push_all also into every peer's SYM_OUT at the same offset. */
static void p2p_tree(struct planner *p, const struct job *j, size_t off, size_t len,
		     struct lfa_ref dst, int push_all)
{
	uint32_t first = p_tree_begin(p);

	for (int k = 0; k < j->n; k++)
		p_ref(p, k == j->r ? ref(LFA_BUF_SEND, off * j->esz) :
		      sref(LFA_BUF_SYM_IN, k, off * j->esz));
	/* in the order r+1, r+2, …: each block's pushes start on a different
	 * link */
	for (int k = 1; push_all && k < j->n; k++)
		p_ref(p, sref(LFA_BUF_SYM_OUT, (j->r + k) % j->n, off * j->esz));
	p_tree_end(p, LFA_STEP_TREE_PUT, first, (uint32_t)j->n, dst, len);
}

/* Copy the whole gathered result from rank r's SYM_OUT: its own block was
 * written there by its own tree, so one launch covers every block. */
static void p2p_unstage_output(struct planner *p, const struct job *j)
{
	p_copy(p, ref(LFA_BUF_RESULT, 0), sref(LFA_BUF_SYM_OUT, j->r, 0), j->bytes);
}

/* The reducing collectives over the symmetric workspace, for groups the tree
 * and put kernels take whole; the rest (pure transport, larger groups) keep
 * the TREE schedules.  n = 1: only a one-shot-sized bucket — the one-shot
 * kernel's degenerate group, one copy launch ending in the completion word (a
 * one-member endpoint runs it when its solo copy is turned off,
 * lfa_coll_ep_test_solo). */
static int plan_p2p(struct planner *p, const struct job *j)
{
	const size_t blk_off = j->moff * j->esz;

	if (!coll_reduces(j->coll) || j->n > LFA_TREE_MAX || j->n > LFA_PUT_MAX ||
	    (j->n == 1 && !oneshot_fits(j)))
		return 0;
	if (oneshot_fits(j)) {
		p_oneshot(p, j->coll == LFA_ALLREDUCE ? LFA_ONESHOT_ALL :
			  j->coll == LFA_REDUCE_SCATTER ? LFA_ONESHOT_SCATTER : j->root,
			  j->n, j->count);
		return 1;
	}
	p2p_stage_input(p, j);
	switch (j->coll) {
	case LFA_ALLREDUCE:
		if (j->bytes * (size_t)j->n <= LFA_SMALL_AG_BYTES) {
			/* one phase: every rank reduces the whole vector */
			p2p_tree(p, j, 0, j->count, ref(LFA_BUF_RESULT, 0), 0);
			p_barrier(p);
			break;
		}
		p2p_tree(p, j, j->moff, j->mlen, sref(LFA_BUF_SYM_OUT, j->r, blk_off), 1);
		p_barrier(p);
		p2p_unstage_output(p, j);
		break;
	case LFA_REDUCE_SCATTER:
		p2p_tree(p, j, j->moff, j->mlen, ref(LFA_BUF_RESULT, 0), 0);
		p_barrier(p);
		break;
	default:        /* LFA_REDUCE */
		p2p_tree(p, j, j->moff, j->mlen, sref(LFA_BUF_SYM_OUT, j->root, blk_off), 0);
		p_barrier(p);
		if (j->r == j->root)
			p2p_unstage_output(p, j);
		break;
	}
	return 1;
}

/* ====================================================================== */
/* entry points                                                            */
/* ====================================================================== */

/* Plan into `p`: 0, -LFA_EINVAL, -LFA_ENOSYS or -LFA_ENOMEM.  Each
 * algorithm's function answers 1 (planned), 0 (not its case: the TREE
 * schedule) or an error. */
static int plan_into(struct planner *p, enum lfa_collective_op coll,
		     enum lfa_coll_algo algo, int r, int n, int root, size_t count,
		     size_t esz)
{
	struct job j = { coll, r, n, root, count, esz, count * esz, 0, 0 };
	int ret;

	if (n < 1 || r < 0 || r >= n || !esz)
		return -LFA_EINVAL;
	if ((coll == LFA_REDUCE || coll == LFA_BROADCAST || coll == LFA_SCATTER) &&
	    (root < 0 || root >= n))
		return -LFA_EINVAL;
	lfa_coll_block(count, n, r, &j.moff, &j.mlen);
	switch (algo) {
	case LFA_ALGO_TREE:
	case LFA_ALGO_RCCL:     /* the RCCL algo is not a schedule */
		ret = 0;
		break;
	case LFA_ALGO_RD:
		ret = plan_rd(p, &j);
		break;
	case LFA_ALGO_TREE_COLL:
		ret = plan_tree_coll(p, &j);
		break;
	case LFA_ALGO_P2P:
		ret = plan_p2p(p, &j);
		break;
	default:
		return -LFA_ENOSYS;
	}
	if (!ret)
		ret = plan_tree(p, &j);
	if (ret < 0)
		return ret;
	return p->nomem ? -LFA_ENOMEM : 0;
}

int lfa_coll_plan(enum lfa_collective_op coll, enum lfa_coll_algo algo,
		  int rank, int nranks, int root, size_t count, size_t esz,
		  struct lfa_step *steps, size_t *nsteps, struct lfa_ref *refs,
		  size_t *nrefs, size_t *tmp_bytes)
{
	struct planner p;
	size_t cap, rcap;
	int ret;

	if (!nsteps || !nrefs || !tmp_bytes)
		return -LFA_EINVAL;
	p_init(&p);
	ret = plan_into(&p, coll, algo, rank, nranks, root, count, esz);
	if (ret != -LFA_EINVAL)
		*tmp_bytes = 0;
	if (!ret) {
		/* what fits is written; the counts are always the plan's */
		cap = steps ? *nsteps : 0;
		rcap = refs ? *nrefs : 0;
		if (cap)
			memcpy(steps, p.steps, (p.n < cap ? p.n : cap) * sizeof(*steps));
		if (rcap)
			memcpy(refs, p.refs, (p.nr < rcap ? p.nr : rcap) * sizeof(*refs));
		*nsteps = p.n;
		*nrefs = p.nr;
		*tmp_bytes = p.tmp;
		if (steps && refs && (p.n > cap || p.nr > rcap))   /* else: size query */
			ret = -LFA_ETOOSMALL;
	}
	p_free(&p);
	return ret;
}

LFA_INTERNAL void plan_free(struct plan *pl)
{
	free(pl->steps);
	free(pl->refs);
	memset(pl, 0, sizeof(*pl));
}

/* The planner's arrays become the plan's, or are freed with `ret` set. */
static int plan_take(struct plan *pl, struct planner *p, int ret)
{
	memset(pl, 0, sizeof(*pl));
	if (!ret && p->nomem)
		ret = -LFA_ENOMEM;
	if (ret) {
		p_free(p);
		return ret;
	}
	pl->steps = p->steps;
	pl->refs = p->refs;
	pl->nsteps = p->n;
	pl->nrefs = p->nr;
	pl->tmp = p->tmp;
	return 0;
}

LFA_INTERNAL int plan_make(struct plan *pl, enum lfa_collective_op coll,
			   enum lfa_coll_algo algo, int rank, int n, int root,
			   size_t count, size_t esz)
{
	struct planner p;

	p_init(&p);
	return plan_take(pl, &p, plan_into(&p, coll, algo, rank, n, root, count, esz));
}

/* ONESHOT -> the items it is defined by: COPY src -> own SYM_IN, BARRIER,
 * TREE of this rank's part over every rank's SYM_IN, BARRIER. */
static void lower_oneshot_step(struct planner *p, const struct lfa_step *st, int r,
			       int n, size_t esz)
{
	size_t moff, mlen;
	uint32_t first;

	lfa_oneshot_part(st, n, r, &moff, &mlen);
	p_copy(p, sref(LFA_BUF_SYM_IN, r, 0), st->src, st->count * esz);
	p_barrier(p);
	if (mlen) {
		first = p_tree_begin(p);
		for (int k = 0; k < (int)st->nsrc; k++)
			p_ref(p, ref_at(k == r ? st->src : sref(LFA_BUF_SYM_IN, k, 0),
					moff * esz));
		p_tree_end(p, LFA_STEP_TREE, first, st->nsrc, st->dst, mlen);
	}
	p_barrier(p);
}

/* Collective items -> grouped SEND/RECV items (transports without
 * collectives).  lower_barrier: BARRIER -> a ring of zero-byte messages,
 * every rank to every other (peer transports, whose sends leave only after
 * the rank's earlier items have completed).  lower_oneshot: ONESHOT -> the
 * items it is defined by, for executors that run all ranks on one stream
 * (the loopback), where one rank's kernel cannot wait for another's. */
LFA_INTERNAL int lower_plan(const struct plan *in, int r, int n, size_t esz,
			    struct plan *out, int lower_barrier, int lower_oneshot)
{
	const struct lfa_ref none = ref(0, 0);
	struct planner p;

	p_init(&p);
	for (size_t i = 0; i < in->nrefs; i++)
		p_ref(&p, in->refs[i]);
	p.tmp = in->tmp;
	for (size_t i = 0; i < in->nsteps; i++) {
		const struct lfa_step *st = &in->steps[i];
		const uint64_t c = st->count;

		if (lower_oneshot && st->type == LFA_STEP_ONESHOT) {
			lower_oneshot_step(&p, st, r, n, esz);
		} else if (lower_barrier && st->type == LFA_STEP_BARRIER) {
			p_ring(&p, p_msg, r, n, fixed(none, 0), fixed(none, 0));
		} else if (st->type == LFA_STEP_ALLTOALL) {
			p_ring(&p, p_xfer, r, n, slots(st->src, c, c), slots(st->dst, c, c));
			p_copy(&p, ref_at(st->dst, (uint64_t)r * c),
			       ref_at(st->src, (uint64_t)r * c), c);
		} else if (st->type == LFA_STEP_ALLGATHER) {
			p_ring(&p, p_xfer, r, n, fixed(st->src, c), slots(st->dst, c, c));
			p_copy(&p, ref_at(st->dst, (uint64_t)r * c), st->src, c);
		} else {
			*push(&p, st->type) = *st;
		}
	}
	return plan_take(out, &p, 0);
}

/* ====================================================================== */
/* plan queries                                                            */
/* ====================================================================== */

LFA_INTERNAL int plan_uses_sym(const struct lfa_step *st, size_t nsteps)
{
	for (size_t i = 0; i < nsteps; i++)
		if (st[i].type == LFA_STEP_BARRIER || st[i].type == LFA_STEP_TREE_PUT ||
		    st[i].type == LFA_STEP_ONESHOT)
			return 1;
	return 0;
}

LFA_INTERNAL size_t sym_region(size_t count, size_t esz)
{
	return (count * esz + 255) & ~(size_t)255;
}

LFA_INTERNAL size_t os_slot(const struct lfa_step *st, int n, size_t esz)
{
	size_t part = st->count;

	if (lfa_oneshot_mode(st) == LFA_ONESHOT_SCATTER)
		part = (st->count + (size_t)n - 1) / (size_t)n;
	return sym_region(part, esz);
}

LFA_INTERNAL size_t plan_sym_need(const struct lfa_step *st, size_t nsteps, int n,
				  size_t count, size_t esz)
{
	size_t need = sym_region(count, esz);

	for (size_t i = 0; i < nsteps; i++)
		if (st[i].type == LFA_STEP_ONESHOT &&
		    2 * (size_t)n * os_slot(&st[i], n, esz) > need)
			need = 2 * (size_t)n * os_slot(&st[i], n, esz);
	return need;
}
