/*
 * bp_layout_check.c -- the carve-up of the bucket planners' workspace pool
 * (re_amd/csrc/host/bp_layout.h) swept over every route and a grid of batch
 * shapes: head offsets, alignment, each region as large as its kernel
 * indexes, no overlap, the total no larger than the size each route reserved
 * before the layout was stated once.  Every region's first and last bytes are
 * written in a buffer of exactly the total, so an overrun is AddressSanitizer's
 * to see (guarded()).  Built and run by tests/test_bp_layout_cpu.py.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include "bp_layout.h"

static long g_bad, g_cases;

#define CHECK(cond)                                                          \
	do {                                                                 \
		if (!(cond) && g_bad++ < 20)                                 \
			printf("FAIL %s: n=%zu nsess=%zu nb=%zu cap=%zu "    \
			       "parts=%#x\n", #cond, n, nsess, nb, cap,      \
			       (unsigned)parts);                             \
	} while (0)

struct region {
	int bit;
	size_t off, need;
};

/* what each route reserved for w->bp before bp_layout.h (batch_dev.c at the
 * commit before it; sgpu_bplan_scratch: plan_buckets.hip:980-989 there) */
static size_t old_scratch(size_t n, size_t nsess, size_t nb, size_t cap)
{
	return bp_al256(nb * cap * 16) + bp_al256(nb * cap * 4) +
	       bp_al256(bp_nscatter(n) * 4) + bp_al256(nsess * 4) +
	       bp_al256(nsess * 32);
}

static size_t old_reserve(size_t n, size_t nsess, size_t nb, size_t cap,
			  enum bp_parts parts)
{
	switch (parts) {
	case BP_RESIDENT:       /* dev_bplanned_issue, batch_dev.c:2067-2070 */
		return BP_HEAD + old_scratch(n, nsess, nb, cap) + n * 4 + 256;
	case BP_RESIDENT_RX:    /* dev_mrxplanned, batch_dev.c:2562-2565 */
		return BP_HEAD + old_scratch(n, nsess, nb, cap) + nb * 8 + n +
		       512;
	case BP_TABLE:          /* dev_mplanned_rtcp, batch_dev.c:1694-1695;
				   dev_msplanned, batch_dev.c:2783-2784 */
		return BP_HEAD + bp_al256(nb * cap * 16) +
		       bp_al256(bp_nscatter(n) * 4);
	case BP_TABLE_RX:       /* dev_mrrxplanned, batch_dev.c:1877-1882;
				   dev_msrxplanned, batch_dev.c:2970-2975 */
		return BP_HEAD + bp_al256(nb * cap * 16) +
		       bp_al256(bp_nscatter(n) * 4) + bp_al256(nb * 8) +
		       bp_al256(n);
	}
	return 0;
}

/*
 * A buffer of exactly `total` bytes behind which a write faults: malloc's
 * under AddressSanitizer, or, past 64 MiB (where the sanitizer's shadow costs
 * tens of milliseconds per buffer and the sweep 18 s), a mapping that ends at
 * a page without access.  *map: what to unmap, or NULL (free the buffer).
 */
#define BIG ((size_t)64 << 20)

static unsigned char *guarded(size_t total, void **map, size_t *len)
{
	const size_t page = (size_t)sysconf(_SC_PAGESIZE);
	unsigned char *m;

	*map = NULL;
	if (total <= BIG)
		return malloc(total);
	*len = (total + page - 1) / page * page + page;
	m = mmap(NULL, *len, PROT_READ | PROT_WRITE,
		 MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
	if (m == MAP_FAILED || mprotect(m + *len - page, page, PROT_NONE))
		return NULL;
	*map = m;
	return m + *len - page - total;
}

static void check(size_t n, size_t nsess, size_t nb, size_t cap,
		  enum bp_parts parts)
{
	const struct bp_layout l = bp_layout(n, nsess, nb, cap, parts);
	const struct region all[] = {
		{BP_TMP, l.tmp, nb * cap * 16},
		{BP_SORTED, l.sorted, nb * cap * 4},
		{BP_AFAIL, l.afail,
		 (n + SGPU_BP_BLOCK * SGPU_BP_PPT - 1) /
		 (SGPU_BP_BLOCK * SGPU_BP_PPT) * 4},
		{BP_SSEG, l.sseg, nsess * 4},
		{BP_SOUT, l.sout, nsess * 32},
		{BP_ORDER, l.order, n * 4},
		{BP_CNT, l.cnt, nb * 8},
		{BP_RS, l.rs, n}};
	const size_t nall = sizeof(all) / sizeof(all[0]);
	size_t end = BP_HEAD, i, first = 1, maplen = 0;
	unsigned char *buf;
	void *map;

	g_cases++;
	CHECK(l.ticket == 0 && l.obins == 64 && l.bcount == 512);
	CHECK(BP_HEAD == 512 + 4 * SGPU_BP_NBMAX && nb <= SGPU_BP_NBMAX);
	CHECK(l.total <= old_reserve(n, nsess, nb, cap, parts));
	buf = guarded(l.total, &map, &maplen);
	if (!buf) {
		printf("no buffer of %zu bytes\n", l.total);
		exit(2);
	}
	memset(buf, 0xa5, BP_HEAD);
	for (i = 0; i < nall; i++) {
		const struct region *r = &all[i];
		const size_t fill = r->need < 64 ? r->need : 64;
		if (!(parts & r->bit)) {
			CHECK(r->off == 0);     /* not used: a NULL pointer */
			continue;
		}
		if (first)
			CHECK(r->off == BP_HEAD);
		first = 0;
		CHECK(r->off % 256 == 0);
		CHECK(r->off >= end);           /* behind the region before */
		end = r->off + r->need;
		CHECK(end <= l.total);
		if (end > l.total)
			continue;
		memset(buf + r->off, (int)i + 1, fill);
		memset(buf + end - fill, (int)i + 1, fill);
	}
	/* nothing a later region wrote reached into an earlier one */
	for (i = 0; i < nall; i++) {
		const struct region *r = &all[i];
		if ((parts & r->bit) && r->off + r->need <= l.total) {
			CHECK(buf[r->off] == i + 1);
			CHECK(buf[r->off + r->need - 1] == i + 1);
		}
	}
	CHECK(buf[0] == 0xa5 && buf[BP_HEAD - 1] == 0xa5);
	if (map)
		munmap(map, maplen);
	else
		free(buf);
}

int main(void)
{
	static const size_t ns[] = {1, 4095, 4096, 4097, 5000, 1u << 20,
				    1u << 26};
	static const size_t nsesss[] = {2, 255, 256, 257, 300, 65536};
	static const size_t nbs[] = {1, 2, 5, 4096};
	static const size_t caps[] = {1024, 2048, 4096};
	static const enum bp_parts parts[] = {BP_RESIDENT, BP_RESIDENT_RX,
					      BP_TABLE, BP_TABLE_RX};
	size_t a, b, c, d, e;

	for (a = 0; a < sizeof(ns) / sizeof(ns[0]); a++)
	for (b = 0; b < sizeof(nsesss) / sizeof(nsesss[0]); b++)
	for (c = 0; c < sizeof(nbs) / sizeof(nbs[0]); c++)
	for (d = 0; d < sizeof(caps) / sizeof(caps[0]); d++)
	for (e = 0; e < sizeof(parts) / sizeof(parts[0]); e++)
		check(ns[a], nsesss[b], nbs[c], caps[d], parts[e]);
	printf("%ld layouts, %ld wrong\n", g_cases, g_bad);
	return g_bad != 0;
}
