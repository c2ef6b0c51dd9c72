/*
 * plan_rtcp_seg_fold.h -- settling an SRTCP unprotect batch over many sessions
 * (HMAC suites) some of whose packets are forged, per (session, SSRC), behind
 * a plan of plan_rtcp_seg.h / plan_rtcp_seg_rx.h that was accepted and whose
 * crypto launch then counted tag misses.  Pure functions over
 * plan_rtcp_seg_rx.h and plan_rx_rule.h, none of their rules said again.
 * Compiles as C (tests/c/rtcp_seg_fold_check.c runs them in the kernel's
 * decomposition against a sequential receiver) and as HIP device code
 * (plan_buckets_rtcp_fold.hip).
 *
 * The SRTCP index travels in the packet and the HMAC covers it with the
 * session's key (srtcp.c:173-201), so the tag verdicts of the first crypto
 * launch hang on no state and are final.  What hangs on them is the replay
 * rule: plan_rtcp_seg_rx.h takes the top before arrival i for
 * max(lix0, mx[i]) "whatever the verdicts before it were", which holds for
 * EALREADY and not for EAUTH -- a forged packet returns before
 * srtp_replay_check (srtcp.c:200-209), never moves the top and never sets a
 * bit.  It does take or open its stream slot (stream_get comes first,
 * srtcp.c:163).
 *
 * So the slots, ranks and positions are the plan's own, and a forged arrival
 * enters the (sum, max) scan with the index -1 (rsfold_ix): never a maximum
 * beside lix0 >= 0, never equal to a 31-bit index.  u[] / mx[] then are the
 * indices and the exclusive prefix maxima of the authentic arrivals alone,
 * rx_replay over them is the receiver's rule unchanged (rsrx_verdict; the
 * verdict of a forged arrival itself means nothing and is not asked for), and
 * the window after the batch takes the authentic maximum (rsfold_smx: a
 * stream forged throughout keeps its record) and the accepted packets' bits.
 *
 * Against the plan that already ran, masking only lowers tops and removes
 * copies: a verdict can move from EALREADY to accepted and in no other way.
 * Such a packet's tag is verified and it was left undeciphered (E clear in its
 * desc word): rsfold_flip names it for the decipher launch.  RX_UNSETTLED (a
 * possible copy older than the look-back, once a forged copy inside it no
 * longer counts) declines the settlement.
 */
#ifndef PLAN_RTCP_SEG_FOLD_H
#define PLAN_RTCP_SEG_FOLD_H

#include "plan_rtcp_seg_rx.h"

/* a packet's result: the receiver's 0 / EALREADY / EAUTH */
enum {
	RSF_OK = 0,
	RSF_DUP = 1,
	RSF_AUTH = 2,
};

/* the index an arrival enters the scan with */
PLAN_FN int64_t rsfold_ix(uint32_t word, int forged)
{
	return forged ? -1 : (int64_t)(word & 0x7fffffffu);
}

/* the scan element of a stream's arrival (rsrx_elem over rsfold_ix): the
 * first one carries its index, the others their distance to the arrival
 * before (pword, pforged) */
PLAN_FN int64_t rsfold_elem(int head, uint32_t word, int forged, uint32_t pword,
			    int pforged)
{
	const int64_t ix = rsfold_ix(word, forged);
	return head ? ix : ix - rsfold_ix(pword, pforged);
}

/* result of arrival i of a stream (RSF_*, or -1: not settled); u[] / mx[] from
 * the scan over rsfold_elem */
PLAN_FN int rsfold_result(const int64_t *u, const int64_t *mx, uint32_t i,
			  uint32_t K, struct rseg_rec st, int forged)
{
	int r;
	if (forged)
		return RSF_AUTH;
	r = rsrx_verdict(u, mx, i, K, st);
	return r == RX_OK ? RSF_OK : r == RX_DUP ? RSF_DUP : -1;
}

/* desc word of a settled authentic packet (rsrx_desc) */
PLAN_FN uint64_t rsfold_desc(int result, uint32_t word)
{
	return rsrx_desc(result == RSF_DUP ? RX_DUP : RX_OK, word);
}

/* the maximum of a stream's authentic indices from its last arrival's u and
 * mx; none authentic: the window's top before the batch, which rseg_top and
 * rsrx_after then leave where it is */
PLAN_FN uint32_t rsfold_smx(struct rseg_rec st, int64_t ulast, int64_t mxlast)
{
	const int64_t m = rx_max(ulast, mxlast);
	return m < 0 ? st.ix : (uint32_t)m;
}

/* the plan that ran left the packet undeciphered (desc0: its E clear) and the
 * settled verdict deciphers it (desc1); encrypted: the suite ciphers SRTCP */
PLAN_FN int rsfold_flip(uint64_t desc0, uint64_t desc1, uint32_t encrypted)
{
	return encrypted && !(desc0 >> 31 & 1u) && (desc1 >> 31 & 1u);
}

/* the byte the settle leaves per packet: the result, and SV_CIPHERED for a
 * packet to decipher (the compact kernels' keystream launch reads it as the
 * verdict byte of a packet to run the keystream over) */
PLAN_FN uint8_t rsfold_byte(int result, int flip)
{
	return (uint8_t)((uint32_t)result << 2 | (flip ? SV_CIPHERED : 0u));
}

PLAN_FN int rsfold_byte_result(uint8_t b)
{
	return b >> 2;
}

#endif
