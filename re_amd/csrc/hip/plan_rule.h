/*
 * plan_rule.h -- the per-packet rules every device planner speculates and
 * verifies with, stated once: the window, header and order checks
 * (srtp_encrypt / srtp_decrypt, src/srtp/srtp.c:183-432), the index
 * (srtp_get_index, misc.c:22-41), the replay window (srtp_replay_check,
 * replay.c:32-62) and the SRTCP per-packet checks (srtcp.c:143-287).
 * Pure functions of scalars: no memory access, no atomics.  Compiles as C
 * (tests/c/plan_rule_check.c runs them against a sequential receiver) and
 * as HIP device code (every planner kernel); the loads, the prefix sums
 * and the out->fail atomics stay with the kernels.
 *
 * A planner assumes packet k of a stream sees s_l = sb = the seq of packet
 * k-1 (the stored s_l for the first), counts the ROC rollovers before it
 * with a prefix sum and checks with plan_order that every packet leaves
 * s_l as the next one assumes; then plan_index under that ROC is exact,
 * and plan_new_first / plan_new_later hold only for a batch whose every
 * index is new and increasing.  A miss of any check rejects the whole plan
 * (SPF_*) and the host plans sequentially.
 */
#ifndef PLAN_RULE_H
#define PLAN_RULE_H

#include <stdint.h>
#include "../srtpgpu.h"

#ifdef __HIPCC__
#define PLAN_FN __host__ __device__ static inline
#else
#define PLAN_FN static inline
#endif

#define PLAN_NOHDR 0xffffffffu          /* sgpu_hdr.hdr_len: unparsable */

/* sgpu_desc() (srtpgpu.h) on the device */
PLAN_FN uint64_t d_desc(uint64_t ix, uint32_t flags)
{
	return (ix & 0xffffull) | ((uint64_t)(uint32_t)(ix >> 16) << 16) |
	       ((uint64_t)flags << 48);
}

/* the index a desc word holds */
PLAN_FN uint64_t d_desc_ix(uint64_t d)
{
	return (d & 0xffffull) | ((d >> 16) & 0xffffffffull) << 16;
}

/* srtp_get_index (misc.c:22-41), including the int wrap of roc +- 1 */
PLAN_FN int32_t plan_v(uint32_t roc, uint32_t s_l, uint32_t seq)
{
	if (s_l < 32768)
		return ((int)seq - (int)s_l > 32768) ? (int32_t)(roc - 1)
						     : (int32_t)roc;
	return ((int)s_l - 32768 > (int)seq) ? (int32_t)(roc + 1)
					     : (int32_t)roc;
}

/* ROC rollover seen by a packet (srtp.c:208-213, 318-321) */
PLAN_FN int plan_wrap(uint32_t seq, uint32_t sb)
{
	return (int)seq - (int)sb <= -32768;
}

/*
 * The packet's window [pos, end) in an arena of asz bytes: SPF_SIZE,
 * SPF_BAD, SPF_CAP.  has_cap: the batch carries buffer capacities (cap is
 * this packet's); need: bytes a protect appends.
 */
PLAN_FN uint32_t plan_window_flags(uint32_t pos, uint32_t end, int has_cap,
				   uint32_t cap, uint64_t asz, uint32_t maxlen,
				   uint32_t need, int prot)
{
	uint32_t f = 0;
	if (end - pos >= maxlen)
		f |= SPF_SIZE;
	if ((pos & 3u) || pos > end || end > asz ||
	    (has_cap && (end > cap || cap > asz)))
		f |= SPF_BAD;
	if (prot && has_cap && (uint64_t)end + need > (uint64_t)cap)
		f |= SPF_CAP;
	return f;
}

/* how a site checks the packet's SSRC against the expected one */
enum {
	PLAN_SSRC_NONE = 0,     /* not here (or nothing to compare with) */
	PLAN_SSRC_PARSED = 1,   /* only a parsable header has an SSRC */
	PLAN_SSRC_ALWAYS = 2,   /* whatever the parse left in hdr.ssrc */
};

/*
 * The packet's header against packet 0's (hl0) and its stream's SSRC:
 * SPF_PARSE, SPF_CLASS, SPF_SSRC.  tag_room: also check that an unprotect
 * has its tag behind the header (L: the window's length).
 */
PLAN_FN uint32_t plan_header_flags(uint32_t hdr_len, uint32_t hl0,
				   uint32_t ssrc, uint32_t ssrc_exp,
				   int ssrc_mode, uint32_t L, uint32_t tag,
				   int tag_room, int prot)
{
	uint32_t f = 0;
	if (hdr_len == PLAN_NOHDR || hl0 == PLAN_NOHDR)
		f |= SPF_PARSE;
	else if (((hdr_len ^ hl0) >> 2) & 3u)
		f |= SPF_CLASS;
	if (ssrc_mode != PLAN_SSRC_NONE && ssrc != ssrc_exp &&
	    (ssrc_mode == PLAN_SSRC_ALWAYS || hdr_len != PLAN_NOHDR))
		f |= SPF_SSRC;
	if (tag_room && !prot && hdr_len != PLAN_NOHDR && L - hdr_len < tag)
		f |= SPF_PARSE;
	return f;
}

/* what a packet does to its stream's (roc, s_l), seen from the speculated
 * s_l = sb */
struct plan_ord {
	uint32_t flags;         /* SPF_TIMEOUT | SPF_ORDER */
	uint32_t wrap;          /* it rolls the ROC over */
};

/*
 * ETIMEDOUT (srtp.c:313-316) and the speculation's own condition: the next
 * packet of the stream sees s_l = seq only if this one left it so
 * (srtp.c:426-427 keeps the larger), which the stream's last packet need
 * not.
 */
PLAN_FN struct plan_ord plan_order(uint32_t seq, uint32_t sb, int last,
				   int prot)
{
	struct plan_ord o;
	o.flags = 0;
	if (!prot && (int)seq - (int)sb > 32768)
		o.flags |= SPF_TIMEOUT;
	o.wrap = (uint32_t)plan_wrap(seq, sb);
	if (!last && !o.wrap && seq < sb)
		o.flags |= SPF_ORDER;
	return o;
}

/* s_l after the stream's last packet (srtp.c:209-213, 426-427) */
PLAN_FN uint32_t plan_s_l_after(uint32_t seq, uint32_t sb, int wrap)
{
	return wrap ? seq : (seq > sb ? seq : sb);
}

struct plan_idx {
	uint64_t ix;            /* the packet's 48-bit index */
	uint32_t fl;            /* its desc flags (SD_*) */
};

/*
 * roc: the stream's ROC after this packet's own rollover.  Sender:
 * srtp.c:215.  Receiver: srtp_get_index from s_l = 0 after a rollover, sb
 * otherwise; where it answers roc +- 1 the trailer ROC differs from the
 * index's high part (SD_ROC_M1 / SD_ROC_P1).
 */
PLAN_FN struct plan_idx plan_index(uint32_t roc, int wrap, uint32_t sb,
				   uint32_t seq, int prot)
{
	struct plan_idx r;
	r.fl = SD_RUN | SD_CIPHER;
	if (prot) {
		r.ix = 65536ull * roc + seq;
	}
	else {
		const int32_t v = plan_v(roc, wrap ? 0u : sb, seq);
		r.ix = seq + (uint64_t)(int64_t)v * 65536ull;
		if ((uint32_t)v != roc)
			r.fl |= (uint32_t)v + 1u == roc ? SD_ROC_P1 : SD_ROC_M1;
	}
	return r;
}

/* receiver: the index of the stream's packet (pseq, seen from s_l = psb)
 * before one whose ROC after its own rollover (wrap) is roc */
PLAN_FN uint64_t plan_prev_index(uint32_t roc, int wrap, uint32_t psb,
				 uint32_t pseq)
{
	return plan_index(roc - (wrap ? 1u : 0u), plan_wrap(pseq, psb), psb,
			  pseq, 0).ix;
}

/* replay, speculated: every packet of the batch is new (replay.c:32-62).
 * The stream's first packet against the stored window ... */
PLAN_FN int plan_new_first(uint64_t ix, uint64_t lix, uint64_t bitmap)
{
	if (ix > lix)
		return 1;
	return lix - ix < 64 && !(bitmap & (1ull << (lix - ix)));
}

/* ... and a later one above its predecessor's index pix, and above the
 * pre-batch lix too: a first packet below lix leaves the window's bits in
 * play (replay.c:53-61), and the final window (plan_win_step over the
 * batch's tail) holds only for indices above it */
PLAN_FN int plan_new_later(uint64_t ix, uint64_t pix, uint64_t lix)
{
	return ix > pix && ix > lix;
}

struct plan_win {
	uint64_t lix, bitmap;
};

/* the replay window after an index known to be accepted (replay.c:32-62) */
PLAN_FN struct plan_win plan_win_step(struct plan_win w, uint64_t ix)
{
	if (ix > w.lix) {
		const uint64_t d = ix - w.lix;
		w.bitmap = d < 64 ? (w.bitmap << d) | 1ull : 1ull;
		w.lix = ix;
	}
	else {
		w.bitmap |= 1ull << (w.lix - ix);
	}
	return w;
}

struct plan_rtcp {
	uint32_t flags;         /* SPF_* */
	uint32_t ix, E;         /* the packet's 31-bit index and E bit */
};

/*
 * SRTCP packet i of a one-stream batch (srtcp.c:31-140 sender, 143-287
 * receiver).  parsed: it has its 8 bytes; L: its length; wflags: its
 * plan_window_flags (SPF_CAP there: ENOMEM, cap_short); word / pword: the
 * E || index word of it and of the packet before it (receiver, pword for
 * i > 0 only).
 */
PLAN_FN struct plan_rtcp plan_rtcp_packet(struct sgpu_rplan_in in, uint32_t i,
					  int parsed, uint32_t ssrc,
					  uint32_t ssrc_exp, uint32_t L,
					  uint32_t wflags, uint32_t word,
					  uint32_t pword)
{
	struct plan_rtcp r;
	r.flags = wflags;               /* plan_window_flags */
	if (!parsed)
		r.flags |= SPF_PARSE;           /* < 8 bytes: EBADMSG */
	else if (ssrc != ssrc_exp)
		r.flags |= SPF_SSRC;
	if (in.prot) {
		r.ix = (in.rtcp_index + i + 1u) & 0x7fffffffu; /* srtcp.c:54 */
		r.E = in.encrypted;
		return r;
	}
	/* srtcp.c:166-172 (and 239-241 for GCM): room for E || index, the
	 * tag, and the GCM tag before them */
	if (L < 8u + 4u + in.tag + (in.gcm ? 16u : 0u))
		r.flags |= SPF_PARSE;
	r.ix = word & 0x7fffffffu;
	r.E = word >> 31;
	if (in.hmac) {
		/* replay (srtcp.c:208-209), speculated: every index new and
		 * increasing, a later one above the pre-batch lix too */
		const int ok = i == 0 ? plan_new_first(r.ix, in.lix, in.bitmap)
				      : plan_new_later(r.ix, pword & 0x7fffffffu,
						       in.lix);
		if (!ok)
			r.flags |= SPF_REPLAY;
	}
	return r;
}

/* an SRTCP packet's desc word */
PLAN_FN uint64_t plan_rtcp_desc(uint32_t ix, uint32_t E)
{
	return ((uint64_t)(ix & 0x7fffffffu)) | ((uint64_t)E << 31) |
	       ((uint64_t)SD_RUN << 48);
}

#endif
