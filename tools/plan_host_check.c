/*
 * plan_host_check.c — the collective planner (lfa_coll_plan.c) on the host
 * alone: no HIP, no liblfa, no Python.  It includes the planner's source so
 * that it reaches the hidden plan_make / lower_plan and the plan queries,
 * supplies lfa_param itself, walks a grid of (collective, algorithm, group
 * size, rank, root, element size, count) and prints one line per
 * (collective, algorithm, n): the return code of the plain case (rank 0,
 * root 0, count n, 4-byte elements), and two digests, each with the plans
 * and cases behind it: `full` over every case of the line, `core` over the
 * cases a short run keeps (core_case).  --core plans the core cases alone
 * and prints `full=-`: the run for the sanitizer build, which would take
 * minutes over the whole grid.  tests/test_plan_host_cpu.py compares the
 * lines with tests/golden/plan_digests.txt, recorded before the planner was
 * rewritten; a schedule that moves by one bit changes its line.
 *
 *   gcc -std=gnu11 -O2 -Wall -Wextra -Werror -Iinclude -Ilibfabric_amd/csrc \
 *       tools/plan_host_check.c -o plan_host_check
 *   ./plan_host_check [--core]         # plan_digests.txt
 *   ./plan_host_check [--core] 65536 131072
 *                                      # plan_digests_knobs.txt: LFA_OS_AG_BYTES,
 *                                      # LFA_OS_RS_BYTES (cached per process);
 *                                      # LFA_ALGO_P2P, n <= LFA_TREE_MAX + 1
 *
 * Also built with -fsanitize=address,undefined -fno-sanitize-recover=all.
 *
 * Digest: FNV-1a's step (xor, then multiply by the 64-bit FNV prime) over
 * 64-bit words, not bytes: byte by byte the whole grid takes two minutes, by
 * words under half a minute.  struct lfa_step is 56 bytes and struct lfa_ref
 * 16, neither with padding, so their raw words are hashed.  Per case:
 * the return code; for a plan nsteps, nrefs, tmp, plan_uses_sym,
 * plan_sym_need and both arrays of the raw plan and of the four
 * lower_plan(lower_barrier, lower_oneshot) outputs; on rank 0 also the public
 * entry's size query and its answer to arrays half as long.  A case's digest
 * is then folded into the line's.
 * Every plan is also checked here: no LFA_BUF_TMP ref reaches past `tmp`.
 */
#include <stdio.h>

#include "lfa_coll_plan.c"

_Static_assert(sizeof(struct lfa_step) == 56, "lfa_step has padding");
_Static_assert(sizeof(struct lfa_ref) == 16, "lfa_ref has padding");

#define CHECK(x)                                                           \
	do {                                                               \
		if (!(x)) {                                                \
			fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, \
				__LINE__, #x, where);                      \
			exit(1);                                           \
		}                                                          \
	} while (0)

static const char *knob_ag, *knob_rs;
static char where[160];

const char *lfa_param(const char *name)
{
	if (!strcmp(name, "LFA_OS_AG_BYTES"))
		return knob_ag;
	if (!strcmp(name, "LFA_OS_RS_BYTES"))
		return knob_rs;
	return NULL;
}

static const char *const coll_name[] = {
	"barrier", "broadcast", "alltoall", "allreduce", "allgather",
	"reduce_scatter", "reduce", "scatter", "gather",
};
static const char *const algo_name[] = {
	"tree", "rd", "rccl", "tree_coll", "p2p", "auto",
};
#define NCOLL ((int)(sizeof(coll_name) / sizeof(coll_name[0])))
#define NALGO ((int)(sizeof(algo_name) / sizeof(algo_name[0])))

static const int group_sizes[] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 31, 32, 33,
				   47, 48, 64, 100, 511, 512, 513, 1100 };
static const size_t elem_sizes[] = { 1, 4, 8 };
/* The core cases: up to this group size every case.  Above it, at root 0
 * with 4-byte elements, the first and the last rank at every count and the
 * other ranks at the fixed counts (not those around the byte bounds); every
 * other (root, element size) pair on every rank at two counts, n + 1 (ragged
 * blocks) and 72 000. */
#define CORE_GRID_MAX 9

#define FNV_BASIS 0xcbf29ce484222325ull
#define FNV_PRIME 0x100000001b3ull

static uint64_t h;      /* the digest of the case being planned */

static uint64_t fnv1a(uint64_t d, uint64_t word)
{
	return (d ^ word) * FNV_PRIME;
}

static void fold(uint64_t v)
{
	h = fnv1a(h, v);
}

/* An array: word i into lane i % 4 (four multiply chains side by side),
 * then the lanes into the digest. */
static void fold_words(const void *p, size_t bytes)
{
	const unsigned char *c = p;
	uint64_t lane[4] = { FNV_BASIS, FNV_BASIS + 1, FNV_BASIS + 2, FNV_BASIS + 3 };
	uint64_t w;

	for (size_t i = 0; i < bytes / 8; i++) {
		memcpy(&w, c + 8 * i, 8);
		lane[i % 4] = fnv1a(lane[i % 4], w);
	}
	for (int l = 0; l < 4; l++)
		fold(lane[l]);
}

/* A TMP ref of `bytes` stays inside the plan's TMP. */
static void tmp_fits(const struct plan *pl, struct lfa_ref r, uint64_t bytes)
{
	if (r.buf == LFA_BUF_TMP && bytes)
		CHECK(r.off + bytes <= pl->tmp);
}

static void check_tmp(const struct plan *pl, int n, size_t esz)
{
	for (size_t i = 0; i < pl->nsteps; i++) {
		const struct lfa_step *s = &pl->steps[i];
		uint64_t c = s->count;

		switch (s->type) {
		case LFA_STEP_SEND:
			tmp_fits(pl, s->src, c);
			break;
		case LFA_STEP_RECV:
			tmp_fits(pl, s->dst, c);
			break;
		case LFA_STEP_COPY:
			tmp_fits(pl, s->dst, c);
			tmp_fits(pl, s->src, c);
			break;
		case LFA_STEP_REDUCE:
			tmp_fits(pl, s->dst, c * esz);
			tmp_fits(pl, s->src, c * esz);
			break;
		case LFA_STEP_TREE:
		case LFA_STEP_TREE_PUT: {
			uint32_t nref = s->nsrc;

			if (s->type == LFA_STEP_TREE_PUT)
				nref += lfa_step_put_extra(s);
			CHECK(s->first + (size_t)nref <= pl->nrefs);
			tmp_fits(pl, s->dst, c * esz);
			for (uint32_t k = 0; k < nref; k++)
				tmp_fits(pl, pl->refs[s->first + k], c * esz);
			break;
		}
		case LFA_STEP_ALLTOALL:
			tmp_fits(pl, s->dst, c * (uint64_t)n);
			tmp_fits(pl, s->src, c * (uint64_t)n);
			break;
		case LFA_STEP_ALLGATHER:
			tmp_fits(pl, s->dst, c * (uint64_t)n);
			tmp_fits(pl, s->src, c);
			break;
		default:
			break;
		}
	}
}

static void fold_plan(const struct plan *pl, int n, size_t count, size_t esz)
{
	check_tmp(pl, n, esz);
	fold(pl->nsteps);
	fold(pl->nrefs);
	fold(pl->tmp);
	fold((uint64_t)plan_uses_sym(pl->steps, pl->nsteps));
	fold(plan_sym_need(pl->steps, pl->nsteps, n, count, esz));
	fold_words(pl->steps, pl->nsteps * sizeof(*pl->steps));
	fold_words(pl->refs, pl->nrefs * sizeof(*pl->refs));
}

/* The public entry: the size query gives the plan's counts, and arrays half
 * as long give -LFA_ETOOSMALL, the same counts and the plan's first items. */
static void fold_public(const struct plan *pl, int coll, int algo, int r, int n,
			int root, size_t count, size_t esz)
{
	size_t ns = 0, nr = 0, tmp = 0, hs = pl->nsteps / 2, hr = pl->nrefs / 2;
	struct lfa_step *steps = calloc(hs ? hs : 1, sizeof(*steps));
	struct lfa_ref *refs = calloc(hr ? hr : 1, sizeof(*refs));
	int ret;

	CHECK(steps && refs);
	ret = lfa_coll_plan(coll, algo, r, n, root, count, esz, NULL, &ns, NULL, &nr,
			    &tmp);
	CHECK(ret == 0 && ns == pl->nsteps && nr == pl->nrefs && tmp == pl->tmp);
	ns = hs;
	nr = hr;
	ret = lfa_coll_plan(coll, algo, r, n, root, count, esz, steps, &ns, refs, &nr,
			    &tmp);
	CHECK(ret == (hs < pl->nsteps || hr < pl->nrefs ? -LFA_ETOOSMALL : 0));
	CHECK(ns == pl->nsteps && nr == pl->nrefs && tmp == pl->tmp);
	fold((uint64_t)ret);
	fold_words(steps, hs * sizeof(*steps));
	fold_words(refs, hr * sizeof(*refs));
	free(steps);
	free(refs);
}

/* One case into h: its return code, and for a plan everything the header
 * lists. */
static int fold_case(int coll, int algo, int r, int n, int root, size_t count,
		     size_t esz)
{
	struct plan pl, low;
	int ret;

	h = FNV_BASIS;
	snprintf(where, sizeof(where), "%s %s n=%d rank=%d root=%d count=%zu esz=%zu",
		 coll_name[coll], algo_name[algo], n, r, root, count, esz);
	ret = plan_make(&pl, coll, algo, r, n, root, count, esz);
	fold((uint64_t)ret);
	if (ret)
		return ret;
	fold_plan(&pl, n, count, esz);
	for (int mode = 0; mode < 4; mode++) {
		CHECK(lower_plan(&pl, r, n, esz, &low, mode >> 1, mode & 1) == 0);
		fold_plan(&low, n, count, esz);
		plan_free(&low);
	}
	if (r == 0)
		fold_public(&pl, coll, algo, r, n, root, count, esz);
	plan_free(&pl);
	return 0;
}

static int cmp_size(const void *a, const void *b)
{
	size_t x = *(const size_t *)a, y = *(const size_t *)b;

	return x < y ? -1 : x > y;
}

/* count·unit on `bound`, one element below and one above. */
static size_t around(size_t *c, size_t k, size_t bound, size_t unit)
{
	size_t on = bound / unit;

	c[k++] = on ? on - 1 : 0;
	c[k++] = on;
	c[k++] = on + 1;
	return k;
}

static int fixed_count(size_t c, int n)
{
	return c <= 1 || c + 1 == (size_t)n || c == (size_t)n || c == (size_t)n + 1 ||
	       c == 7 || c == 1000 || c == 70001 || c == 72000;
}

/* Is the case one of the core cases?  (CORE_GRID_MAX) */
static int core_case(int n, int r, int root, size_t esz, size_t count)
{
	if (n <= CORE_GRID_MAX)
		return 1;
	if (root != 0 || esz != 4)
		return count == (size_t)n + 1 || count == 72000;
	return r == 0 || r == n - 1 || fixed_count(count, n);
}

/* A line's digest with the plans and cases behind it. */
struct tally {
	uint64_t digest;
	size_t plans, cases;
};

static void tally_case(struct tally *t, int ret)
{
	t->digest = fnv1a(t->digest, h);
	t->cases++;
	t->plans += !ret;
}

static size_t counts_for(size_t *c, int n, size_t esz)
{
	const size_t bounds[] = { LFA_SMALL_AG_BYTES, LFA_OS_AG_BYTES_DEFAULT,
				  LFA_OS_RS_BYTES, lfa_os_ag_bytes(), lfa_os_rs_bytes(),
				  (size_t)16 << 20 };
	const size_t fixed[] = { 0, 1, (size_t)n - 1, (size_t)n, (size_t)n + 1, 7,
				 1000, 70001, 72000 };
	size_t k = 0, u = 0;

	for (size_t i = 0; i < sizeof(fixed) / sizeof(fixed[0]); i++)
		c[k++] = fixed[i];
	for (size_t i = 0; i < sizeof(bounds) / sizeof(bounds[0]); i++) {
		k = around(c, k, bounds[i], esz);
		k = around(c, k, bounds[i], esz * (size_t)n);
	}
	/* the per-block bound: count·esz / n on LFA_TREE_SKEW_MIN */
	k = around(c, k, (size_t)LFA_TREE_SKEW_MIN * (size_t)n, esz);
	qsort(c, k, sizeof(*c), cmp_size);
	for (size_t i = 0; i < k; i++)
		if (!u || c[i] != c[u - 1])
			c[u++] = c[i];
	return u;
}

static int ranks_for(int *ranks, int n)
{
	int rem = n - (int)pof2_floor((uint64_t)n), k = 0, u = 0;
	const int pick[] = { 0, 1, 2 * rem - 1, 2 * rem, n - 1 };

	if (n <= 64) {
		for (int r = 0; r < n; r++)
			ranks[r] = r;
		return n;
	}
	for (int i = 0; i < 5; i++)
		if (pick[i] >= 0 && pick[i] < n)
			ranks[k++] = pick[i];
	for (int i = 0; i < k; i++) {
		int dup = 0;

		for (int j = 0; j < u; j++)
			dup |= ranks[j] == ranks[i];
		if (!dup)
			ranks[u++] = ranks[i];
	}
	return u;
}

int main(int argc, char **argv)
{
	const int core_only = argc > 1 && !strcmp(argv[1], "--core");
	const int knobs = argc - core_only > 2;
	int ranks[64];
	size_t counts[64];

	if (knobs) {
		knob_ag = argv[1 + core_only];
		knob_rs = argv[2 + core_only];
	}
	printf("# one-shot bounds: ag %zu rs %zu\n", lfa_os_ag_bytes(),
	       lfa_os_rs_bytes());
	for (int coll = 0; coll < NCOLL; coll++)
	for (int algo = 0; algo < NALGO; algo++)
	for (size_t gi = 0; gi < sizeof(group_sizes) / sizeof(group_sizes[0]); gi++) {
		const int n = group_sizes[gi], nranks = ranks_for(ranks, n);
		struct tally core = { FNV_BASIS, 0, 0 }, full = { FNV_BASIS, 0, 0 };
		int rc, ret;

		/* the knobs are read by LFA_ALGO_P2P alone and only for groups
		 * up to LFA_TREE_MAX: their run stops one size past it */
		if (knobs && (algo != LFA_ALGO_P2P || n > LFA_TREE_MAX + 1))
			continue;
		/* the plain case, then the -LFA_EINVAL answers, once each */
		const struct { int root; size_t esz; } once[] = {
			{ 0, 4 }, { -1, 4 }, { n, 4 }, { 0, 0 },
		};
		rc = 0;
		for (int i = 0; i < 4; i++) {
			ret = fold_case(coll, algo, 0, n, once[i].root, (size_t)n,
					once[i].esz);
			if (!i)
				rc = ret;
			tally_case(&core, ret);
			tally_case(&full, ret);
		}
		for (size_t ei = 0; ei < sizeof(elem_sizes) / sizeof(elem_sizes[0]); ei++) {
			const size_t esz = elem_sizes[ei], nc = counts_for(counts, n, esz);

			for (int root = 0; root < n; root += n > 1 ? n - 1 : 1)
			for (int ri = 0; ri < nranks; ri++)
			for (size_t ci = 0; ci < nc; ci++) {
				const int is_core = core_case(n, ranks[ri], root, esz,
							      counts[ci]);

				if (core_only && !is_core)
					continue;
				ret = fold_case(coll, algo, ranks[ri], n, root, counts[ci],
						esz);
				tally_case(&full, ret);
				if (is_core)
					tally_case(&core, ret);
			}
		}
		printf("%s %s n=%d rc=%d core=%zu/%zu:%016llx", coll_name[coll],
		       algo_name[algo], n, rc, core.plans, core.cases,
		       (unsigned long long)core.digest);
		if (core_only)
			printf(" full=-\n");
		else
			printf(" full=%zu/%zu:%016llx\n", full.plans, full.cases,
			       (unsigned long long)full.digest);
	}
	return 0;
}
