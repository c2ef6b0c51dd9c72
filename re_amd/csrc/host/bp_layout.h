/*
 * bp_layout.h -- how a call of the bucket planners (plan_buckets*.hip) cuts up
 * the workspace pool w->bp: byte offsets only, no pointers, so it is checked
 * on the CPU (tests/c/bp_layout_check.c).  batch_dev.c bp_take reserves
 * `total` bytes and turns the offsets into device pointers.
 *
 * The head is the same for every route and stays zero between calls (the
 * finish launches leave it so; bp_take zeroes a new pool's):
 *   0    ticket words (the fold's last-workgroup ticket)
 *   64   obins: packets per length bin
 *   512  bcount: entries per bucket, SGPU_BP_NBMAX words
 * Behind it, each 256-byte aligned, the regions a route names in this order:
 *   tmp     nb x cap bucket entries of 16 bytes
 *   sorted  nb x cap packet indices by session
 *   afail   one fail word per scatter workgroup
 *   sseg    per session: start | count << 16
 *   sout    per session: its state after the batch (struct sgpu_sstate)
 *   order   the crypto launch order, n words
 *   cnt     receive planners: late, duplicates per bucket
 *   rs      receive planners: one verdict byte per packet
 */
#ifndef BP_LAYOUT_H
#define BP_LAYOUT_H

#include <stddef.h>
#include <stdint.h>
#include "../srtpgpu.h"         /* SGPU_BP_* */

#define BP_HEAD (512u + 4u * SGPU_BP_NBMAX)
#define BP_SSTATE 32u           /* sizeof(struct sgpu_sstate) */

enum {
	BP_TMP = 1, BP_SORTED = 2, BP_AFAIL = 4, BP_SSEG = 8, BP_SOUT = 16,
	BP_ORDER = 32, BP_CNT = 64, BP_RS = 128
};

/* the regions each route uses */
enum bp_parts {
	/* resident states, in order (dev_bplanned_issue) */
	BP_RESIDENT = BP_TMP | BP_SORTED | BP_AFAIL | BP_SSEG | BP_SOUT |
		      BP_ORDER,
	/* resident states, receive (dev_mrxplanned) */
	BP_RESIDENT_RX = BP_TMP | BP_SORTED | BP_AFAIL | BP_SSEG | BP_SOUT |
			 BP_CNT | BP_RS,
	/* the host's stream tables (dev_msplanned, dev_mplanned_rtcp) */
	BP_TABLE = BP_TMP | BP_AFAIL,
	/* ... their receive routes (dev_msrxplanned, dev_mrrxplanned), and the
	 * settle of forged SRTCP packets behind either SRTCP route
	 * (mrfold_settle) */
	BP_TABLE_RX = BP_TMP | BP_AFAIL | BP_CNT | BP_RS
};

struct bp_layout {
	size_t ticket, obins, bcount;           /* the head */
	size_t tmp, sorted, afail, sseg, sout, order, cnt, rs;  /* 0: not used */
	size_t total;                           /* bytes to reserve */
};

static inline size_t bp_al256(size_t x)
{
	return (x + 255) & ~(size_t)255;
}

/* scatter workgroups of n packets */
static inline size_t bp_nscatter(size_t n)
{
	return (n + SGPU_BP_BLOCK * SGPU_BP_PPT - 1) /
	       (SGPU_BP_BLOCK * SGPU_BP_PPT);
}

static inline struct bp_layout bp_layout(size_t n, size_t nsess, size_t nb,
					 size_t cap, enum bp_parts parts)
{
	struct bp_layout l = {.ticket = 0, .obins = 64, .bcount = 512};
	size_t o = BP_HEAD;
#define BP_PART(bit, field, bytes)                                           \
	if (parts & (bit)) {                                                 \
		l.field = o;                                                 \
		o += bp_al256(bytes);                                        \
	}
	BP_PART(BP_TMP, tmp, nb * cap * 16)
	BP_PART(BP_SORTED, sorted, nb * cap * 4)
	BP_PART(BP_AFAIL, afail, bp_nscatter(n) * 4)
	BP_PART(BP_SSEG, sseg, nsess * 4)
	BP_PART(BP_SOUT, sout, nsess * BP_SSTATE)
	BP_PART(BP_ORDER, order, n * 4)
	BP_PART(BP_CNT, cnt, nb * 8)
	BP_PART(BP_RS, rs, n)
#undef BP_PART
	l.total = o;
	return l;
}

#endif
