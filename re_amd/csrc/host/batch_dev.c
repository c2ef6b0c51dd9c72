/*
 * batch_dev.c -- fully device-resident batches (srtp_*_batch_dev):
 * packets, positions and stream state stay in HBM and the plan runs on the
 * device.  The routes (batch_async.c after_host / run_dev pick among them):
 *
 * route              planner                          state     call
 * RTP, one session
 *  fz_issue/_finish  k_ctr_fused.h (in or before the  host      issue/finish
 *                    crypto launch)
 *  dp_issue/_finish  srtp_kernels.hip k_plan_*        host      issue/finish
 *  dev_rxplanned     plan_rx.hip                      host      sync only
 *  dev_splanned      plan_streams.hip                 host      issue/finish
 *  dev_srxplanned    plan_streams_rx.hip              host      sync only
 * RTP, many sessions
 *  dev_mplanned      plan_buckets.hip, plan_multi.hip resident  issue/finish
 *  dev_mrxplanned    plan_buckets_rx.hip              resident  sync only
 *  dev_msplanned     plan_buckets_rtp_streams.hip     table     sync only
 *  dev_msrxplanned   plan_buckets_rtp_streams_rx.hip  table     sync only
 * SRTCP, one session
 *  dev_planned_rtcp  srtp_kernels.hip (k_rp_plan,     host      sync only
 *                    k_plan_rtcp)
 *  dev_splanned_rtcp plan_streams_rtcp.hip            host      sync only
 * SRTCP, many sessions
 *  dev_mplanned_rtcp plan_buckets_rtcp.hip            table     sync only
 *  dev_mrrxplanned   plan_buckets_rtcp_rx.hip         table     sync only
 *  (mrfold_settle     plan_buckets_rtcp_fold.hip: behind either, a batch with
 *                     forged packets under srtp_gpu_tune mrfold)
 *
 * state: where the plan reads the stream states -- host: passed in with the
 * launch; resident: the table in HBM (sgpu_sst_*); table: the host's stream
 * tables, uploaded by the call (struct tab_layout).  call: an issue/finish
 * route is a struct dcall between its launches (*_issue) and its completion
 * (*_finish), so the synchronous calls (dev_call) and the asynchronous
 * tickets (batch_async.c) share it; a sync-only route synchronises itself.
 * Where a call's arrays lie in the workspace pools: struct ws_layout
 * (srtp_int.h), struct fz_layout for w->fz, bp_layout.h for w->bp.
 */
#include <errno.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "re_mem.h"
#include "re_mbuf.h"
#include "re_srtp.h"
#include "re_srtp_batch.h"
#include "re_rtcp_batch.h"
#include "../srtpgpu.h"
#include "../hip/plan_rx_rule.h"
#include "bp_layout.h"
#include "fault.h"
#include "pool.h"
#include "srtp_int.h"

/* ---- what the planners below share ------------------------------------- */

/* the crypto launch over a call's windows and its workspace layout: every
 * packet, nothing guarded; the call sites name what differs */
static struct sgpu_compact compact_of(const struct srtp_batch_dev *d,
				      const struct ws_layout *L)
{
	return (struct sgpu_compact){
		.pos = d->pos, .end = L->es, .hdr = L->hdr, .desc = L->desc,
		.compmap = L->cm, .n = (uint32_t)d->n, .verdict = L->verdict,
		.save = L->save, .nfail = L->nfail};
}

/* a rejected single-stream plan: -2 gated by the chained call before
 * (nothing ran, nothing counted), else -1 */
static int plan_rejected(uint32_t fail, unsigned ns0)
{
	if (fail & SPF_PRED)
		return -2;
	if ((fail & SPF_SSRC) && !ns0)
		__atomic_store_n(&g_fresh_multi, 1, __ATOMIC_RELAXED);
	count(&g_cnt_rejects, 1);
	return -1;
}

/* stream state from a fold the device settled */
static void fold_apply(struct srtp *s, const struct sgpu_fold_out *fo)
{
	struct srtp_stream *st = &s->streams[0];
	st->s_l = (uint16_t)fo->s_l;
	st->replay_rtp.lix = fo->lix;
	st->replay_rtp.bitmap = fo->bitmap;
	count(&g_cnt_devfolds, 1);
}

/* behind a call's undo launches (err: what queueing them returned): the
 * original ends back, one synchronisation; -1 (nothing modified, the host
 * takes over) or errno */
static int undone(int err, const struct srtp_batch_dev *d, const uint32_t *es)
{
	if (!err)
		err = sgpu_memcpy_d2d(d->end, es, d->n * 4, d->stream);
	if (!err)
		err = sgpu_stream_sync(d->stream);
	return err ? err : -1;
}

/* the same behind a plan that wrote no result (its commit or finish launch
 * is guarded by the miss count): the ends never moved */
static int undo_synced(int err, void *stream)
{
	if (!err)
		err = sgpu_stream_sync(stream);
	return err ? err : -1;
}

/* an SRTCP call's undo launch: its crypto launch C again over the one class
 * SRTCP has (AES-CM: 2, the cipher region starts at byte 8; GCM: 0) */
static int undo_rtcp(const struct srtp_batch_dev *d, struct sgpu_compact C,
		     const struct comp *c0)
{
	C.undo = 1;
	return sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				(int)c0->nr, c0->mode == SGPU_MODE_GCM ? 0 : 2, 0,
				d->stream);
}

/* the streams a batch opened, appended in first-appearance order
 * (stream_new, stream.c:45-67); returns the slots of the table after the
 * batch, of which the caller advances the touched ones */
static unsigned streams_append(struct srtp *s, const struct sgpu_splan_out *tab)
{
	const unsigned nst = tab->nst < SRTP_MAX_STREAMS ? tab->nst
							  : SRTP_MAX_STREAMS;
	unsigned k;
	for (k = s->nstreams; k < nst; k++) {
		memset(&s->streams[k], 0, sizeof(s->streams[k]));
		s->streams[k].ssrc = tab->ssrc[k];
	}
	if (tab->nst > s->nstreams)
		s->nstreams = tab->nst;
	return nst;
}

/* ---- one stream, the separate planner (srtp_gpu_tune noplanfuse) ------ */

/* k_parse, k_plan_*, the compact crypto launch, the verdict fold and the
 * results: the launches (no host synchronisation) */
static int dp_issue(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &s->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t T = gcm ? 16u : c0->tag_len;
	const uint32_t need = prot ? (gcm ? 16u : (T > 4 ? T : 4u)) : 0u;
	/* pl: plan out | plan scratch | fold out | fold scratch */
	const size_t foff = (sizeof(struct sgpu_plan_out) + (n / 256 + 8) * 4 +
			     63) & ~63ul;
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 12,
		.vs = n * 9 + 72, .cm = 4,
		.pl = foff + 64 + (n / 256 + 4) * 20, .es = n * 4};
	struct ws_layout L;
	struct sgpu_plan_out *po, *po_d;
	struct sgpu_fold_out *fo_d;
	uint32_t *scr, *fscr;
	void *stream = d->stream;       /* NULL: the default (null) stream */
	int err;

	k->foff = foff;
	err = ws_layout_reserve(w, n, &z, &L);
	if (err)
		return err;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	scr = (uint32_t *)(w->pl.d + sizeof(*po));
	fo_d = (struct sgpu_fold_out *)(w->pl.d + foff);
	fscr = (uint32_t *)(w->pl.d + foff + 64);

	plan_in(&k->in, s, (uint32_t)n, prot, T, need);
	{
		/* one launch: parse + end copy + zeroed counters + comp map */
		struct sgpu_prologue pro = {
			.end_copy = L.es, .z0 = L.nfail, .z1 = (uint32_t *)po_d,
			.nz0 = 1, .nz1 = (uint32_t)(sizeof(*po) / 4),
			.cm_out = L.cm, .cm = c0->dev};
		k->in.zeroed = 1;
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, L.hdr, NULL, (uint32_t)n, 0,
					  &pro, stream);
	}
	k->in.pred = k->pred;   /* the gate check rides in k_plan_count */
	if (!err)
		err = sgpu_plan_rtp(&k->in, L.hdr, d->pos, L.es, d->cap,
				    d->arena_size, L.desc, scr, po_d, stream);
	if (!err) {
		struct sgpu_compact C = compact_of(d, &L);
		C.uniform = 1;
		C.flist = L.flist;
		err = run_classes(d->arena, d->arena_size, C, c0,
				  po_d, prot, stream);
	}
	/* unprotect: the verdict fold queued behind the kernels (nothing to
	 * do without a miss), so a forged packet neither gates the next
	 * chained call nor waits for the host (sgpu_fold_rtp) */
	k->devfold = !prot && !g_env.nodevfold;
	if (!err && k->devfold)
		err = sgpu_fold_rtp(1, L.nfail, &k->in, L.hdr, L.desc, L.verdict,
				    L.es, d->pos, d->end, d->err, gcm, fscr, fo_d,
				    stream);
	/* results, gate word and the miss count next to the plan: one
	 * launch, one copy into pinned memory */
	if (!err)
		err = sgpu_plan_finish(&po_d->fail, L.es, d->end, d->err,
				       (uint32_t)n,
				       prot ? (int32_t)T : -(int32_t)T, L.nfail,
				       k->gate, &po_d->nfail,
				       k->devfold ? &fo_d->fail : NULL, stream);
	if (!err && k->devfold)
		err = sgpu_fold_rtp(2, L.nfail, &k->in, L.hdr, L.desc, L.verdict,
				    L.es, d->pos, d->end, d->err, gcm, fscr, fo_d,
				    stream);
	/* plan out and fold out in one copy */
	if (!err)
		err = sgpu_memcpy_d2h(po, po_d, k->devfold ? foff + sizeof(*fo_d)
							  : sizeof(*po), stream);
	return err;
}

/* ... after its launches completed (as dev_planned_finish) */
static int dp_finish(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const size_t n = d->n;
	const unsigned ns0 = s->nstreams;
	const struct sgpu_plan_out *po = (const struct sgpu_plan_out *)w->pl.h;
	const struct sgpu_fold_out *fo =
		(const struct sgpu_fold_out *)(w->pl.h + k->foff);
	const uint32_t nfail = po->nfail;
	struct ws_layout L;
	struct sgpu_compact C;
	struct srtp_stream old;
	int r;

	k->pfail = po->fail;
	if (po->fail)
		return plan_rejected(po->fail, ns0);
	count(&g_cnt_dplans, 1);
	if (nfail)
		count(&g_cnt_misses, nfail);
	plan_apply(s, po, prot, n, &old);
	if (!nfail)
		return 0;
	/* a forged packet: the verdicts were folded on the device behind the
	 * kernels (dp_issue), the outcome came back with the plan.  The
	 * kernels already left each forged packet as srtp_decrypt does (HMAC:
	 * the ciphertext restored, the ROC over the tag; GCM: decrypted in
	 * place); the fold checks that the speculated rollovers and indices
	 * hold under the true s_l and writes the EAUTH results, s_l and the
	 * replay window (sgpu_fold_rtp). */
	if (!prot && k->devfold && !fo->fail) {
		fold_apply(s, fo);
		return 0;
	}
	count(&g_cnt_folds, 1);
	/* undo on the device, fold on the host engine */
	ws_layout_get(w, n, &L);
	C = compact_of(d, &L);
	C.undo = 1;
	C.uniform = 1;
	r = undone(run_classes(d->arena, d->arena_size, C, &s->rtp,
			       (struct sgpu_plan_out *)w->pl.d, prot, d->stream),
		   d, L.es);
	if (r == -1)
		plan_unapply(s, ns0, &old);
	return r;
}


/* ---- one stream, planned inside the crypto launch (k_ctr_fused.h) ----- */

#define FZ_HEAD 64u             /* ticket word, padded */

/*
 * Single-stream batch planned by the decoupled look-back plan of
 * k_ctr_fused.h (srtpgpu.h struct sgpu_fused), k->fused:
 *
 * 1  AES-CM: inside its crypto launch -- one launch parses, plans and
 *    encrypts / decrypts.  A rejected plan: every processed packet undone
 *    (sgpu_fused_undo), the ends restored.
 * 2  AES-GCM, and AES-CM with srtp_gpu_tune lplan: k_lp_plan plans the batch
 *    in a launch of its own -- hdr, es, desc, the plan out with the class
 *    guards skip[], the results of every packet planned -- and the lean
 *    crypto kernel runs behind it, guarded by skip[] and out->fail (AES-CM:
 *    k_ctr_fast_any) or by out->fail (GCM: k_gcmu), counting its tag misses
 *    into out->nfail.  A rejected plan wrote no byte of the arena (the
 *    crypto launch did nothing): only the ends are put back.
 *
 * With no forged packet nothing else runs on the device; forged packets
 * get their ciphertext back (k_ctr_refix_list; GCM leaves them decrypted)
 * and the device verdict fold (sgpu_fold_rtp) once the plan out showed a
 * miss (fz_finish).  An asynchronous call sets its chained gate word with
 * the plan out (plan_out_back), so no host round trip is needed.  A
 * rejected plan or a fold the device cannot settle: undone, and -1
 * (k->pfail: the plan's SPF_* bits, 0 for a fold) -- the caller plans on
 * the host, as for the separate device planner.
 *
 * w->fz: ticket | (plan out, fold out) x 2 | look-back words
 */
#define FZ_FO_OFF ((sizeof(struct sgpu_plan_out) + 63u) & ~(size_t)63)
#define FZ_SLOT (FZ_FO_OFF + 64u)
#define FZ_BYTES(nblk) (FZ_HEAD + 2 * FZ_SLOT + (size_t)(nblk) * 8)

/* the pieces of w->fz a call uses: its slot (par) and the other one */
struct fz_layout {
	uint32_t *ticket;
	struct sgpu_plan_out *out;      /* this call's plan out ... */
	struct sgpu_fold_out *fo;       /* ... and fold out */
	struct sgpu_plan_out *out_next; /* the next call's: zeroed by this */
	unsigned long long *agg;        /* look-back words */
	struct sgpu_plan_out *out_h;    /* pinned mirrors of out and fo */
	struct sgpu_fold_out *fo_h;
};

static struct fz_layout fz_layout_get(const struct ws *w, uint32_t par)
{
	const size_t off = FZ_HEAD + (size_t)par * FZ_SLOT;
	const size_t next = FZ_HEAD + (size_t)(par ^ 1) * FZ_SLOT;
	return (struct fz_layout){
		.ticket = (uint32_t *)w->fz.d,
		.out = (struct sgpu_plan_out *)(w->fz.d + off),
		.fo = (struct sgpu_fold_out *)(w->fz.d + off + FZ_FO_OFF),
		.out_next = (struct sgpu_plan_out *)(w->fz.d + next),
		.agg = (unsigned long long *)(w->fz.d + FZ_HEAD + 2 * FZ_SLOT),
		.out_h = (struct sgpu_plan_out *)(w->fz.h + off),
		.fo_h = (struct sgpu_fold_out *)(w->fz.h + off + FZ_FO_OFF)};
}

/* the fused / one-launch planners' workspace state (w->fz for nblk
 * workgroups), zeroed on a new pool, an epoch wrap or srtp_gpu_tune fzepoch
 * (a test hook, one-shot for whichever thread's launch comes next: the
 * look-back words are zeroed with it, so words of an epoch used since the
 * last zeroing can never match) */
static int fz_prepare(struct ws *w, uint32_t nblk, void *stream)
{
	int err = pool_reserve(w, &w->fz, FZ_BYTES(nblk));
	const long e = __atomic_exchange_n(&g_env.fzepoch, 0,
					   __ATOMIC_RELAXED);
	if (err)
		return err;
	if (e > 0 && e <= 0xffff)
		w->fz_d = NULL;
	if (w->fz_d != w->fz.d || w->fz_epoch == 0 ||
	    w->fz_epoch > 0xffffu) {
		err = sgpu_memset(w->fz.d, 0, w->fz.cap, stream);
		if (err)
			return err;
		w->fz_d = w->fz.d;
		w->fz_epoch = 1;
		w->fz_tbase = 0;
		w->fz_par = 0;
	}
	if (e > 0 && e <= 0xffff)
		w->fz_epoch = (uint32_t)e;
	return 0;
}

/* the workspace's pinned completion word for synchronous single-stream
 * calls (srtp_gpu_tune syncspin), once */
static int sync_word(struct ws *w)
{
	if (!w->sy_word) {
		w->sy_word = fi_sgpu_host_alloc(4);
		if (w->sy_word)
			*w->sy_word = 0;
	}
	return w->sy_word != NULL;
}

/* wait for a synchronous call: its post's completion word when it has one
 * (spinning, the stream asked now and then whether it stopped without
 * it: a fault), else the stream */
static int sync_wait(struct dcall *k, void *stream)
{
	unsigned long i;
	if (!k->spin)
		return sgpu_stream_sync(stream);
	for (i = 1;; i++) {
		int q;
		if (__atomic_load_n(k->w->sy_word, __ATOMIC_ACQUIRE) == k->spin)
			return 0;
		if (i & 1023) {
			__builtin_ia32_pause();
			continue;
		}
		q = sgpu_stream_query(stream);
		if (q == EAGAIN)
			continue;
		if (__atomic_load_n(k->w->sy_word, __ATOMIC_ACQUIRE) == k->spin)
			return 0;
		return q ? q : EIO;
	}
}

/* a single-stream call's plan out back to its pinned mirror, behind the
 * crypto launch; an asynchronous call also sets its chained gate word
 * (out->fail || out->nfail: the plan failed or a tag did not verify --
 * forged packets' restore and verdict fold run when the call is waited
 * for, as for a synchronous call, and a chained call queued behind one
 * with misses is gated and re-run; the zero-miss fold launches cost every
 * call ~25 us, a miss costs the call behind it a host round trip) */
static int plan_out_back(struct dcall *k, struct sgpu_plan_out *out,
			 void *host, void *stream)
{
	const int sync = k->sync;
	int err = 0;
	k->devfold = 0;
	if (!g_env.nopost) {
		/* a synchronous call with srtp_gpu_tune syncspin: waited for
		 * by the post's completion word, not a stream synchronisation */
		uint32_t *done = NULL;
		if (sync && g_env.syncspin && sync_word(k->w))
			done = k->w->sy_word;
		k->spin = done ? ++k->w->sy_seq : 0;
		if (k->spin == 0 && done)
			k->spin = ++k->w->sy_seq;       /* never 0 */
		return sgpu_plan_post(out, host, sizeof(*out),
				      sync ? NULL : k->gate, done, k->spin,
				      stream);
	}
	if (!sync && k->gate)
		err = sgpu_plan_finish(&out->fail, NULL, NULL, NULL, 0, 0,
				       &out->nfail, k->gate, NULL, NULL, stream);
	if (!err)
		err = sgpu_memcpy_d2h(host, out, sizeof(*out), stream);
	return err;
}

/* the launches (no host synchronisation) */
static int fz_issue(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	const struct comp *c0 = &s->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;      /* k->fused == 2 only */
	const size_t n = d->n;
	const uint32_t T = gcm ? 16u : c0->tag_len;
	const uint32_t need = prot ? (gcm ? 16u : (T > 4 ? T : 4u)) : 0u;
	const uint32_t B = sgpu_fused_block();
	const uint32_t nblk = (uint32_t)((n + B - 1) / B);
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 9 + 72, .cm = 4, .pl = 64 + (n / 256 + 4) * 20,
		.es = n * 4, .es_first = 1};
	struct ws *w = k->w;
	struct sgpu_fused *F = &k->fz;
	struct ws_layout L;
	struct fz_layout Z;
	void *stream = d->stream;
	int err;

	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = fz_prepare(w, nblk, stream);
	if (err)
		return err;
	k->foff = w->fz_par;
	Z = fz_layout_get(w, w->fz_par);

	memset(F, 0, sizeof(*F));
	plan_in(&F->in, s, (uint32_t)n, prot, T, need);
	F->in.zeroed = 1;
	F->in.pred = k->pred;   /* the chained call before: its gate word */
	F->pos = d->pos;
	F->end = d->end;
	F->cap = d->cap;
	F->err = d->err;
	F->es = L.es;
	F->hdr = L.hdr;
	F->desc = L.desc;
	if (!prot) {
		F->save = L.save;
		F->verdict = L.verdict;
		F->flist = gcm ? NULL : L.flist;
	}
	F->out = Z.out;
	F->out_next = Z.out_next;
	F->cm_out = L.cm;
	F->agg = Z.agg;
	F->ticket = Z.ticket;
	F->tbase = w->fz_tbase;
	F->epoch = w->fz_epoch;
	F->comp = c0->dev;
	F->delta = prot ? (int32_t)T : -(int32_t)T;
	err = k->fused == 1 ? sgpu_run_fused(d->arena, d->arena_size, F,
					     (int)c0->nr, stream)
			    : sgpu_run_fzplan(d->arena, d->arena_size, F, stream);
	if (err) {
		w->fz_d = NULL;         /* counters unknown: from zero next time */
		return err;
	}
	w->fz_tbase += F->ntickets;
	w->fz_epoch++;
	w->fz_par ^= 1;
	if (k->fused == 2) {
		/* the crypto launch behind the plan's guards */
		struct sgpu_compact C = {
			.pos = d->pos, .end = F->es, .hdr = F->hdr,
			.desc = F->desc, .compmap = F->cm_out, .n = (uint32_t)n,
			.verdict = F->verdict, .save = F->save,
			.nfail = &F->out->nfail, .uniform = gcm ? 1 : 2,
			.guard = gcm ? &F->out->fail : F->out->skip,
			.flist = F->flist, .gfail = gcm ? NULL : &F->out->fail};
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : -1, prot, stream);
		if (err)
			return err;
	}
	return plan_out_back(k, F->out, Z.out_h, stream);
}

/* ... after its launches completed (as dev_planned_finish) */
static int fz_finish(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	const int lean = k->fused == 2;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	const struct comp *c0 = &s->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;      /* lean only */
	const size_t n = d->n;
	const unsigned ns0 = s->nstreams;
	struct ws *w = k->w;
	struct sgpu_fused *F = &k->fz;
	const struct fz_layout Z = fz_layout_get(w, (uint32_t)k->foff);
	const struct sgpu_plan_out *po = Z.out_h;
	void *stream = d->stream;
	struct srtp_stream old;
	int err = 0;

	k->pfail = po->fail;
	if (po->fail) {
		/* no work that counts: nothing (gated) or undone */
		if (!lean)
			sgpu_prof_void(F->prof_id);
		if (plan_rejected(po->fail, ns0) == -2)
			return -2;      /* every workgroup did nothing */
		if (po->fail & (SPF_BAD | SPF_SLOW))
			w->fz_d = NULL; /* ticket / look-back state from zero */
		if (po->fail & SPF_SLOW)
			count(&g_cnt_lbtimeout, 1);
		if (!lean)
			goto undo;
		if (g_env.times)
			fprintf(stderr, "re_srtp plan n=%zu %s: rejected "
				"(SPF %#x)\n", n, prot ? "protect" : "unprotect",
				po->fail);
		/* the crypto launch did nothing: only the ends the plan wrote
		 * go back */
		return undone(0, d, F->es);
	}
	plan_apply(s, po, prot, n, &old);
	count(lean ? &g_cnt_lplans : &g_cnt_fused, 1);
	if (!po->nfail)
		return 0;
	count(&g_cnt_misses, po->nfail);
	if (!g_env.nodevfold) {
		/* forged packets: ciphertext back (GCM leaves them decrypted),
		 * verdicts folded on the device; its outcome comes back in one
		 * copy */
		if (!gcm)
			err = sgpu_fused_refix(d->arena, d->arena_size, F,
					       (int)c0->nr, stream);
		if (!err)
			err = sgpu_fold_rtp(0, &F->out->nfail, &F->in, F->hdr,
					    F->desc, F->verdict, F->es, d->pos,
					    d->end, d->err, gcm,
					    (uint32_t *)(w->pl.d + 64), Z.fo,
					    stream);
		if (!err)
			err = sgpu_memcpy_d2h(Z.fo_h, Z.fo, sizeof(*Z.fo),
					      stream);
		if (!err)
			err = sgpu_stream_sync(stream);
		if (err)
			return err;
		k->devfold = 1;
	}
	if (k->devfold && !Z.fo_h->fail) {
		fold_apply(s, Z.fo_h);
		return 0;
	}
	/* the fold cannot be settled on the device (or nodevfold): undo --
	 * forged packets still decrypted are re-encrypted with the rest --
	 * and fold on the host */
	count(&g_cnt_folds, 1);
	plan_unapply(s, ns0, &old);
 undo:
	if (gcm) {
		struct sgpu_compact C = {
			.pos = d->pos, .end = F->es, .hdr = F->hdr,
			.desc = F->desc, .compmap = F->cm_out, .n = (uint32_t)n,
			.verdict = F->verdict, .save = F->save,
			.nfail = &F->out->nfail, .undo = 1, .uniform = 1};
		err = run_classes(d->arena, d->arena_size, C, c0, F->out, prot,
				  stream);
	}
	else if (lean || po->hl0 != 0xffffffffu) {
		F->shift = (po->hl0 >> 2) & 3u;
		err = sgpu_fused_undo(d->arena, d->arena_size, F, (int)c0->nr,
				      prot, stream);
	}
	return undone(err, d, F->es);
}

/* ---- one stream: which planner, and the synchronous calls ------------- */

/* 1: the plan inside the crypto launch, 2: the one-launch planner in front
 * of the lean kernels, 0: the separate planner (struct dcall fused) */
static int planned_kind(const struct srtp *s)
{
	if (g_env.noplanfuse)
		return 0;
	return s->rtp.mode == SGPU_MODE_CTR && !g_env.lplan ? 1 : 2;
}

/* single-stream RTP batch planned and processed on the device: the
 * launches (no host synchronisation) */
int dev_planned_issue(struct dcall *k)
{
	k->fused = planned_kind(k->sessv[0]);
	return k->fused ? fz_issue(k) : dp_issue(k);
}

/* ... after its launches completed: 0 / errno, -1 not plannable or a
 * forged packet the host must fold (nothing modified), -2 gated by the
 * chained call before (nothing modified) */
int dev_planned_finish(struct dcall *k)
{
	return k->fused ? fz_finish(k) : dp_finish(k);
}

/* a synchronous device-planned call: issue, wait, finish (*pfail: a
 * rejected plan's SPF_* bits).  timed: the call may be waited for by its
 * post's completion word (sync_wait), and where its host time goes is
 * counted (counters sync_ns_issue / _wait / _finish) */
static inline int dev_call(int op, struct srtp **sessv, size_t nsess,
			   struct srtp_batch_dev *d, int radix,
			   int (*issue)(struct dcall *),
			   int (*finish)(struct dcall *), int timed,
			   uint32_t *pfail)
{
	struct dcall k;
	uint64_t t0, t1, t2;
	int err;
	memset(&k, 0, sizeof(k));
	k.op = op;
	k.sessv = sessv;
	k.nsess = nsess;
	k.d = *d;
	k.sync = 1;
	k.radix = radix;
	k.w = ws_get();
	*pfail = 0;
	if (!k.w)
		return ENOMEM;
	t0 = timed ? mono_ns() : 0;
	err = issue(&k);
	t1 = timed ? mono_ns() : 0;
	if (!err)
		err = timed ? sync_wait(&k, d->stream)
			    : sgpu_stream_sync(d->stream);
	t2 = timed ? mono_ns() : 0;
	if (err) {
		*pfail = k.pfail;       /* -1 from the issue: why (MPF_MULTI) */
		return err;
	}
	err = finish(&k);
	if (timed) {
		count(&g_cnt_sync_calls, 1);
		count(&g_ns_sync_issue, t1 - t0);
		count(&g_ns_sync_wait, t2 - t1);
		count(&g_ns_sync_finish, mono_ns() - t2);
	}
	*pfail = k.pfail;
	return err;
}

/* synchronous: -1 not plannable (nothing modified; *pfail: why, 0 for a
 * forged packet the host must fold), else 0 / errno */
int dev_planned(int op, struct srtp *s, struct srtp_batch_dev *d,
		       uint32_t *pfail)
{
	return dev_call(op, &s, 1, d, 0, dev_planned_issue, dev_planned_finish,
			planned_kind(s) == 1, pfail);
}

/* ---- one stream, reordered / duplicated arrivals (plan_rx.hip) -------- */

/*
 * The host twin of the device receive planner: the same rule
 * (hip/plan_rx_rule.h) in the same decomposition -- aggregates of `block`
 * packets, a scan of the aggregates, u[] / Mx[] per packet, the settle
 * pass with its look-back across blocks -- so small block / lookback
 * values exercise every boundary of plan_rx.hip on the CPU.
 */
int srtp_rx_plan_host(const struct srtp_stream_state *st0, const uint16_t *seq,
		      size_t n, uint32_t block, uint32_t lookback,
		      uint64_t *ix, int32_t *err, struct srtp_stream_state *st1,
		      uint32_t *fail)
{
	const size_t nb = block ? (n + block - 1) / block : 0;
	struct rx_agg *agg, total = rx_identity();
	int64_t *u, *mx, H0, lix0, lix, Mn, u0 = 0;
	uint64_t bitmap;
	size_t b, i;
	int bump = 0;

	if (!st0 || !seq || !n || !block || !ix || !err || !st1 || !fail ||
	    n > UINT32_MAX)
		return EINVAL;
	*st1 = *st0;
	*fail = 0;
	/* the rule computes in signed 64 bits: a window at a sign-extended
	 * index (ROC 2^31 and above, misc.c:40) is not settled, as in
	 * dev_rxplanned */
	if (st0->replay_rtp_lix >> 62) {
		*fail = SPF_REPLAY;
		return 0;
	}
	agg = fi_malloc(nb * sizeof(*agg));
	u = fi_malloc(n * sizeof(*u));
	mx = fi_malloc(n * sizeof(*mx));
	if (!agg || !u || !mx) {
		free(agg);
		free(u);
		free(mx);
		return ENOMEM;
	}
	/* seed: a fresh stream takes seq[0] as s_l (stream_get_seq) */
	H0 = (int64_t)(((uint64_t)st0->roc << 16) |
		       (st0->s_l_set ? st0->s_l : seq[0]));
	lix0 = (int64_t)st0->replay_rtp_lix;
	if (rx_step(H0, seq[0], &u0, &bump)) {
		*fail = SPF_TIMEOUT;
		goto out;
	}
#define RX_ELEM(i) rx_elem((i) ? rx_sdiff16(seq[i], seq[(i) - 1]) : u0)
	/* 1. per-block aggregates */
	for (b = 0; b < nb; b++) {
		struct rx_agg a = rx_identity();
		for (i = b * block; i < (b + 1) * (size_t)block && i < n; i++)
			a = rx_combine(a, RX_ELEM(i));
		agg[b] = a;
	}
	/* 2. exclusive scan of the aggregates */
	for (b = 0; b < nb; b++) {
		const struct rx_agg a = agg[b];
		agg[b] = total;
		total = rx_combine(total, a);
	}
	/* 3. indices and exclusive prefix maxima, block by block */
	for (b = 0; b < nb; b++) {
		struct rx_agg run = agg[b];
		for (i = b * block; i < (b + 1) * (size_t)block && i < n; i++) {
			mx[i] = run.m;
			run = rx_combine(run, RX_ELEM(i));
			u[i] = run.s;
		}
	}
#undef RX_ELEM
	/* 4. settle; 5. the state after the batch */
	Mn = rx_max(H0, total.m);
	lix = rx_max(lix0, total.m);
	bitmap = rx_bitmap_base(lix, lix0, st0->replay_rtp_bitmap);
	for (i = 0; i < n; i++) {
		const int r = rx_settle(u, mx, (uint32_t)i, seq[i], lookback, H0,
					lix0, st0->replay_rtp_bitmap, 0);
		if (r == RX_UNSETTLED) {
			*fail = SPF_ORDER;
			goto out;
		}
		ix[i] = (uint64_t)u[i];
		err[i] = r == RX_DUP ? EALREADY : 0;
		if (r == RX_OK)
			bitmap |= rx_bit(lix, u[i]);
	}
	st1->roc = (uint32_t)((uint64_t)Mn >> 16);
	st1->s_l = (uint16_t)((uint64_t)Mn & 0xffffu);
	st1->s_l_set = 1;
	st1->replay_rtp_lix = (uint64_t)lix;
	st1->replay_rtp_bitmap = bitmap;
 out:
	free(agg);
	free(u);
	free(mx);
	return 0;
}

/* a rejected one-stream unprotect plan the receive planner may settle:
 * only the arrival order or a replayed index was in its way */
int rx_eligible(int op, const struct srtp *s, uint32_t pfail)
{
	return op == OP_RTP_DEC && !g_env.norxplan && s->nstreams <= 1 &&
	       pfail && !(pfail & ~(uint32_t)(SPF_ORDER | SPF_REPLAY));
}

/*
 * What the two one-session receive routes (dev_rxplanned: one stream;
 * dev_srxplanned: several) share, a call between rx1_run and its tail.
 * Both planners take the same arrays; in and the plan out are their own
 * structs (srx: struct sgpu_srxplan_in / _out, else sgpu_rxplan_in / _out),
 * of which the shared code reads only the words named here.
 */
struct rx1 {
	int srx;
	const struct comp *c0;
	const struct srtp_batch_dev *d;
	struct ws *w;
	const void *in;
	size_t scr, outsz;      /* bytes: the planner's scratch, its plan out */
	size_t o_nfail, o_skip; /* in the plan out: the crypto launches' miss
				   counter, skip[4] (fail is its first word) */
	/* rx1_run's */
	struct sgpu_compact C;  /* the crypto launch */
	uint32_t *fail_d, *skip_d;
	const void *out;        /* the plan out, pinned */
};

/*
 * The parse prologue, the plan, the general descriptor-driven crypto launch
 * guarded by its verdict, the guarded results (commit), one copy back, one
 * synchronisation.  hcopy: pos | end | err go to w->ms.h as well.  0: x->out
 * holds the outcome, with the forged packets still to look at; -1: not
 * settled (nothing modified); errno.
 */
static int rx1_run(struct rx1 *x, int hcopy)
{
	const struct comp *c0 = x->c0;
	const struct srtp_batch_dev *d = x->d;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t T = gcm ? 16u : c0->tag_len;
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4, .pl = 64 + x->outsz, .es = n * 4};
	struct ws_layout L;
	struct ws *w = x->w;
	void *stream = d->stream;
	uint8_t *out_d;
	int err;

	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = pool_reserve(w, &w->mscr, x->scr);
	if (!err && hcopy)
		err = pool_reserve(w, &w->ms, n * 12);
	if (err)
		return err;
	x->out = w->pl.h;
	out_d = w->pl.d;
	x->fail_d = (uint32_t *)out_d;
	x->skip_d = (uint32_t *)(out_d + x->o_skip);
	{
		/* one launch: parse + end copy + zeroed plan out + comp map */
		struct sgpu_prologue pro = {
			.end_copy = L.es, .z0 = (uint32_t *)out_d,
			.nz0 = (uint32_t)(x->outsz / 4), .cm_out = L.cm,
			.cm = c0->dev};
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, L.hdr, NULL, (uint32_t)n, 0,
					  &pro, stream);
	}
	if (!err)
		err = x->srx ? sgpu_splan_rx(x->in, L.hdr, d->pos, L.es, d->cap,
					     d->arena_size, L.desc, w->mscr.d,
					     x->scr, (void *)out_d, stream)
			     : sgpu_plan_rx(x->in, L.hdr, d->pos, L.es, d->cap,
					    d->arena_size, L.desc, w->mscr.d,
					    x->scr, (void *)out_d, stream);
	/* the general kernels (EALREADY packets: MAC only): AES-CM picks the
	 * header class from skip[], GCM has one */
	x->C = compact_of(d, &L);
	x->C.nfail = (uint32_t *)(out_d + x->o_nfail);
	x->C.uniform = 1;
	x->C.guard = gcm ? x->fail_d : x->skip_d;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &x->C, c0->mode,
				       (int)c0->nr, gcm ? 0 : -1, 0, stream);
	if (!err)
		err = x->srx ? sgpu_splan_rx_commit((void *)out_d, L.hdr,
						    w->mscr.d, L.es, d->pos,
						    d->end, d->err, (uint32_t)n,
						    T, stream)
			     : sgpu_plan_rx_commit((void *)out_d, L.hdr,
						   w->mscr.d, L.es, d->pos,
						   d->end, d->err, (uint32_t)n,
						   T, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->pl.h, out_d, x->outsz, stream);
	if (!err && hcopy) {
		err = sgpu_memcpy_d2h(w->ms.h, d->pos, n * 4, stream);
		if (!err)
			err = sgpu_memcpy_d2h(w->ms.h + n * 4, d->end, n * 4,
					      stream);
		if (!err)
			err = sgpu_memcpy_d2h(w->ms.h + n * 8, d->err, n * 4,
					      stream);
	}
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err || !*(const uint32_t *)x->out)
		return err;
	if (g_env.times)
		fprintf(stderr, "re_srtp %srx plan n=%zu: not settled "
			"(SPF %#x)\n", x->srx ? "streams " : "", n,
			*(const uint32_t *)x->out);
	return -1;
}

/* a forged packet: undo on the device (the results were not written), fold
 * on the host engine.  AES-CM: one guarded launch per header class, GCM:
 * one */
static int rx1_undo(struct rx1 *x)
{
	const struct comp *c0 = x->c0;
	const struct srtp_batch_dev *d = x->d;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	int q, err = 0;

	x->C.undo = 1;
	for (q = 0; q < (gcm ? 1 : 4) && !err; q++) {
		x->C.guard = gcm ? x->fail_d : &x->skip_d[q];
		err = sgpu_run_compact(d->arena, d->arena_size, &x->C, c0->mode,
				       (int)c0->nr, q, 0, d->stream);
	}
	return undo_synced(err, d->stream);
}

/*
 * One-stream unprotect batch behind such a rejection, planned by
 * sgpu_plan_rx (rx1_run).  hpos / hend / herr: host arrays the results are
 * copied down to as well (host-window calls), or NULL.
 * 0: done, the stream advanced; -1: not settled, or a forged packet
 * (undone) -- nothing modified, the caller's fallback continues; errno.
 */
int dev_rxplanned(struct srtp *s, struct srtp_batch_dev *d, uint32_t *hpos,
		  uint32_t *hend, int32_t *herr)
{
	const struct comp *c0 = &s->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t T = gcm ? 16u : c0->tag_len;
	const struct srtp_stream *st0 = s->nstreams ? &s->streams[0] : NULL;
	struct sgpu_rxplan_in in;
	struct rx1 x = {
		.c0 = c0, .d = d, .w = ws_get(), .in = &in,
		.scr = sgpu_plan_rx_scratch((uint32_t)n),
		.outsz = sizeof(struct sgpu_rxplan_out),
		.o_nfail = offsetof(struct sgpu_rxplan_out, nfail),
		.o_skip = offsetof(struct sgpu_rxplan_out, skip)};
	const struct sgpu_rxplan_out *ro;
	const struct ws *w = x.w;
	struct srtp_stream *st;
	int err;

	if (!w)
		return ENOMEM;
	/* the rule computes in signed 64 bits (an imported window) */
	if (st0 && (st0->replay_rtp.lix >> 62))
		return -1;
	memset(&in, 0, sizeof(in));
	in.n = (uint32_t)n;
	in.fresh = !st0 || !st0->s_l_set;
	in.ssrc_any = !st0;
	in.ssrc = st0 ? st0->ssrc : 0;
	in.roc = st0 ? st0->roc : 0;
	in.s_l = st0 ? st0->s_l : 0;
	in.lix = st0 ? st0->replay_rtp.lix : 0;
	in.bitmap = st0 ? st0->replay_rtp.bitmap : 0;
	in.tag = T;
	in.maxlen = SGPU_CACHED_MAX(c0->mode);
	in.hmac = !gcm;
	in.lookback = RX_LOOKBACK;
	in.zeroed = 1;
	err = rx1_run(&x, hpos != NULL);
	if (err)
		return err;
	ro = x.out;
	if (ro->nfail) {
		count(&g_cnt_misses, ro->nfail);
		count(&g_cnt_folds, 1);
		return rx1_undo(&x);
	}
	if (!s->nstreams) {
		memset(&s->streams[0], 0, sizeof(s->streams[0]));
		s->streams[0].ssrc = ro->ssrc0;
		s->nstreams = 1;
	}
	st = &s->streams[0];
	st->s_l_set = 1;
	st->roc = ro->roc;
	st->s_l = (uint16_t)ro->s_l;
	st->replay_rtp.lix = ro->lix;
	st->replay_rtp.bitmap = ro->bitmap;
	if (hpos) {
		memcpy(hpos, w->ms.h, n * 4);
		memcpy(hend, w->ms.h + n * 4, n * 4);
		memcpy(herr, w->ms.h + n * 8, n * 4);
	}
	count(&g_cnt_rxplans, 1);
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	return 0;
}

/* ---- one session, several streams (plan_streams.hip) ------------------ */

static void splan_in(struct sgpu_splan_in *in, const struct srtp *s,
		     uint32_t n, int prot, uint32_t T, uint32_t need)
{
	unsigned k;
	memset(in, 0, sizeof(*in));
	in->n = n;
	in->prot = (uint32_t)prot;
	in->tag = T;
	in->need = need;
	in->maxlen = SGPU_CACHED_MAX(s->rtp.mode);
	in->nst = s->nstreams;
	for (k = 0; k < s->nstreams; k++) {
		const struct srtp_stream *x = &s->streams[k];
		in->st[k].ssrc = x->ssrc;
		in->st[k].roc = x->roc;
		in->st[k].s_l = x->s_l;
		in->st[k].flags = SST_EXISTS | (x->s_l_set ? SST_SL_SET : 0);
		in->st[k].lix = x->replay_rtp.lix;
		in->st[k].bitmap = x->replay_rtp.bitmap;
	}
}

/* stream states after an accepted plan: streams with packets in the batch
 * advance, new SSRCs are appended in first-appearance order (stream_new,
 * stream.c:45-67) */
static void splan_apply(struct srtp *s, const struct sgpu_splan_out *po,
			int prot)
{
	unsigned k;
	for (k = 0; k < po->nst && k < SRTP_MAX_STREAMS; k++) {
		struct srtp_stream *x = &s->streams[k];
		if (!po->cnt[k])
			continue;
		if (k >= s->nstreams) {
			memset(x, 0, sizeof(*x));
			x->ssrc = po->ssrc[k];
		}
		x->s_l_set = 1;
		x->roc += po->wraps[k];
		x->s_l = (uint16_t)po->s_l_last[k];
		if (!prot)
			x->replay_rtp = plan_replay(&x->replay_rtp, po->tail_ix[k],
						    po->cnt[k]);
	}
	if (po->nst > s->nstreams)
		s->nstreams = po->nst;
}

/* the launches (no host synchronisation) */
int dev_splanned_issue(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &s->rtp;
	const size_t n = d->n;
	const uint32_t T = c0->mode == SGPU_MODE_GCM ? 16u : c0->tag_len;
	const uint32_t need = prot ? (c0->mode == SGPU_MODE_GCM ? 16u :
			      (T > 4 ? T : 4u)) : 0u;
	const size_t scr = sgpu_splan_scratch((uint32_t)n);
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 12,
		.vs = n * 5 + 64, .cm = 4,
		.pl = sizeof(struct sgpu_splan_out) + 64, .es = n * 4};
	struct ws_layout L;
	struct sgpu_splan_out *po, *po_d;
	void *stream = d->stream;
	int err;

	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = pool_reserve(w, &w->mscr, scr);
	if (err)
		return err;
	po = (struct sgpu_splan_out *)w->pl.h;
	po_d = (struct sgpu_splan_out *)w->pl.d;

	splan_in(&k->sin, s, (uint32_t)n, prot, T, need);
	{
		struct sgpu_prologue pro = {
			.end_copy = L.es, .z0 = L.nfail, .z1 = (uint32_t *)po_d,
			.nz0 = 1, .nz1 = (uint32_t)(sizeof(*po) / 4),
			.cm_out = L.cm, .cm = c0->dev};
		k->sin.zeroed = 1;
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, L.hdr, NULL, (uint32_t)n, 0,
					  &pro, stream);
	}
	if (!err && k->pred)
		err = sgpu_gate_pred(k->pred, &po_d->base.fail, stream);
	if (!err)
		err = sgpu_splan_rtp(&k->sin, L.hdr, d->pos, L.es, d->cap,
				     d->arena_size, L.desc, w->mscr.d, scr, po_d,
				     stream);
	if (!err) {
		struct sgpu_compact C = compact_of(d, &L);
		C.uniform = 1;
		err = run_classes(d->arena, d->arena_size, C, c0,
				  &po_d->base, prot, stream);
	}
	if (!err)
		err = sgpu_plan_finish(&po_d->base.fail, L.es, d->end, d->err,
				       (uint32_t)n,
				       prot ? (int32_t)T : -(int32_t)T, L.nfail,
				       k->gate, &po_d->base.nfail, NULL, stream);
	if (!err)
		err = sgpu_memcpy_d2h(po, po_d, sizeof(*po), stream);
	return err;
}

/* ... after its launches completed: 0 / errno, -1 not plannable or a
 * forged packet (undone on the device; the host folds), -2 gated by the
 * chained call before (nothing modified) */
int dev_splanned_finish(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp *s = k->sessv[0];
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &s->rtp;
	const size_t n = d->n;
	const struct sgpu_splan_out *po = (const struct sgpu_splan_out *)w->pl.h;
	struct sgpu_splan_out *po_d = (struct sgpu_splan_out *)w->pl.d;
	const uint32_t nfail = po->base.nfail;
	struct ws_layout L;
	struct sgpu_compact C;

	k->pfail = po->base.fail;
	if (po->base.fail) {
		if (po->base.fail & SPF_PRED)
			return -2;
		count(&g_cnt_rejects, 1);
		return -1;
	}
	count(&g_cnt_splans, 1);
	if (!s->nstreams && po->nst <= 1)
		__atomic_store_n(&g_fresh_multi, 0, __ATOMIC_RELAXED);
	if (!nfail) {
		splan_apply(s, po, prot);
		return 0;
	}
	count(&g_cnt_misses, nfail);
	count(&g_cnt_folds, 1);
	/* a forged packet: undo on the device, fold on the host engine */
	ws_layout_get(w, n, &L);
	C = compact_of(d, &L);
	C.undo = 1;
	C.uniform = 1;
	return undone(run_classes(d->arena, d->arena_size, C, c0, &po_d->base,
				  prot, d->stream), d, L.es);
}

/* synchronous: -1 not plannable (*pfail: why) or folded on the host (0)
 * -- nothing modified --, else 0 / errno */
int dev_splanned(int op, struct srtp *s, struct srtp_batch_dev *d,
		 uint32_t *pfail)
{
	return dev_call(op, &s, 1, d, 0, dev_splanned_issue,
			dev_splanned_finish, 0, pfail);
}

/* ---- one session, several streams, reordered / duplicated arrivals ---- */
/* (plan_streams_rx.hip) */

/* a rejected per-stream unprotect plan the receive planner may settle: only
 * the arrival order or a replayed index inside some stream was in its way */
int srx_eligible(int op, size_t nsess, const struct srtp_batch_dev *d,
		 uint32_t pfail)
{
	return op == OP_RTP_DEC && nsess == 1 && !d->sess && !g_env.nosrxplan &&
	       pfail && !(pfail & ~(uint32_t)(SPF_ORDER | SPF_REPLAY));
}

/*
 * One-session unprotect batch over several SSRCs behind such a rejection,
 * planned by sgpu_splan_rx (rx1_run); then the streams the batch opened are
 * appended in first-appearance order and every touched stream takes its
 * record after the batch.  0: done; -1: not settled, or a forged packet
 * (undone) -- nothing modified, the caller's fallback continues; errno.
 */
int dev_srxplanned(struct srtp *s, struct srtp_batch_dev *d)
{
	const struct comp *c0 = &s->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t T = gcm ? 16u : c0->tag_len;
	struct sgpu_srxplan_in in;
	struct rx1 x = {
		.srx = 1, .c0 = c0, .d = d, .w = ws_get(), .in = &in,
		.scr = sgpu_splan_rx_scratch((uint32_t)n),
		.outsz = sizeof(struct sgpu_srxplan_out),
		.o_nfail = offsetof(struct sgpu_srxplan_out, tab.base.nfail),
		.o_skip = offsetof(struct sgpu_srxplan_out, tab.base.skip)};
	const struct sgpu_srxplan_out *ro;
	unsigned k, nst;
	int err;

	if (!x.w)
		return ENOMEM;
	/* the rule computes in signed 64 bits (an imported window) */
	for (k = 0; k < s->nstreams; k++)
		if (s->streams[k].replay_rtp.lix >> 62)
			return -1;
	memset(&in, 0, sizeof(in));
	splan_in(&in.s, s, (uint32_t)n, 0, T, 0);
	in.s.zeroed = 1;
	in.hmac = !gcm;
	in.lookback = RX_LOOKBACK;
	err = rx1_run(&x, 0);
	if (err)
		return err;
	ro = x.out;
	/* a forged packet: the host engine counts the misses and the one fold,
	 * as it does without this planner */
	if (ro->tab.base.nfail)
		return rx1_undo(&x);
	nst = streams_append(s, &ro->tab);
	for (k = 0; k < nst; k++) {
		struct srtp_stream *st = &s->streams[k];
		const struct sgpu_rtp_rec *a = &ro->after[k];
		if (!ro->cnt[k])
			continue;
		st->roc = a->roc;
		st->s_l = (uint16_t)a->sl;
		st->s_l_set = 1;
		st->replay_rtp.lix = (uint64_t)a->lhi << 32 | a->llo;
		st->replay_rtp.bitmap = (uint64_t)a->bhi << 32 | a->blo;
	}
	count(&g_cnt_srxplans, 1);
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	return 0;
}

/* the SRTCP plan input of a batch of n packets on session s */
static void rplan_in(struct sgpu_rplan_in *in, const struct srtp *s,
		     uint32_t n, int prot)
{
	const struct comp *c0 = &s->rtcp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const uint32_t T = c0->tag_len;             /* 0 for GCM */
	memset(in, 0, sizeof(*in));
	in->n = n;
	in->prot = (uint32_t)prot;
	in->ssrc_any = !s->nstreams;
	in->ssrc = s->nstreams ? s->streams[0].ssrc : 0;
	in->rtcp_index = s->nstreams ? s->streams[0].rtcp_index : 0;
	in->lix = s->nstreams ? s->streams[0].replay_rtcp.lix : 0;
	in->bitmap = s->nstreams ? s->streams[0].replay_rtcp.bitmap : 0;
	in->tag = T;
	in->gcm = (uint32_t)gcm;
	in->hmac = (uint32_t)c0->has_hmac;
	in->encrypted = (uint32_t)(gcm ? c0->encrypted : c0->has_aes);
	in->need = 4u + T + (gcm ? 16u : 0u);
	in->maxlen = SGPU_CACHED_MAX(c0->mode);
}

/* the stream (stream.c:45-67) and its SRTCP state after an accepted
 * plan; *old: the state before */
static void rplan_apply(struct srtp *s, const struct sgpu_plan_out *po,
			int prot, size_t n, struct srtp_stream *old)
{
	if (!s->nstreams) {
		memset(&s->streams[0], 0, sizeof(s->streams[0]));
		s->streams[0].ssrc = po->ssrc0;
		s->nstreams = 1;
	}
	*old = s->streams[0];
	if (prot)
		s->streams[0].rtcp_index =
			(s->streams[0].rtcp_index + (uint32_t)n) & 0x7fffffffu;
	else if (s->rtcp.has_hmac)
		s->streams[0].replay_rtcp =
			plan_replay(&s->streams[0].replay_rtcp, po->tail_ix, n);
}

/*
 * A single-stream SRTCP call behind its synchronisation (dev_lplanned_rtcp,
 * dev_planned_rtcp).  A rejected plan -- the crypto launch C and the results
 * did nothing -- is -1 with its SPF_* bits in *pfail.  Else the stream
 * advances; with a forged packet the batch is undone on the device, the
 * stream put back and the fold left to the host engine (-1).
 */
static int rplanned_done(struct srtp *s, const struct srtp_batch_dev *d,
			 const struct sgpu_plan_out *po, int prot,
			 struct sgpu_compact C, const uint32_t *es,
			 uint32_t *pfail)
{
	const unsigned ns0 = s->nstreams;
	struct srtp_stream old;
	int err;

	if (po->fail) {
		count(&g_cnt_rejects, 1);
		*pfail = po->fail;
		return -1;
	}
	count(&g_cnt_rplans, 1);
	rplan_apply(s, po, prot, d->n, &old);
	if (!po->nfail)
		return 0;
	count(&g_cnt_misses, po->nfail);
	count(&g_cnt_folds, 1);
	C.uniform = s->rtcp.mode == SGPU_MODE_GCM ? 0 : 1;
	err = undone(undo_rtcp(d, C, &s->rtcp), d, es);
	if (err == -1) {
		s->streams[0] = old;
		s->nstreams = ns0;
	}
	return err;
}

/*
 * Single-stream SRTCP batch planned in one launch (k_rp_plan: the parse,
 * every check of k_plan_rtcp, desc) in front of the single-key crypto
 * kernel, which it guards with out->fail and whose misses it counts in
 * out->nfail, then the guarded results; one copy and one
 * synchronisation.  -1: not plannable (nothing modified) or a forged
 * packet (undone), else 0 / errno.
 */
static int dev_lplanned_rtcp(int op, struct srtp *s, struct srtp_batch_dev *d,
			     uint32_t *pfail)
{
	const int prot = op == OP_RTCP_ENC;
	const struct comp *c0 = &s->rtcp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t grow = 4u + c0->tag_len + (gcm ? 16u : 0u);
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4, .es = n * 4, .es_first = 1};
	struct ws_layout L;
	struct fz_layout Z;
	struct sgpu_compact C;
	struct sgpu_rfused R;
	struct sgpu_plan_out *po, *po_d;
	void *stream = d->stream;
	struct ws *w = ws_get();
	int err;

	if (!w)
		return ENOMEM;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = fz_prepare(w, 1, stream);
	if (err)
		return err;
	Z = fz_layout_get(w, w->fz_par);
	po = Z.out_h;
	po_d = Z.out;
	memset(&R, 0, sizeof(R));
	rplan_in(&R.in, s, (uint32_t)n, prot);
	R.pos = d->pos;
	R.end = d->end;
	R.cap = d->cap;
	R.err = d->err;
	R.es = L.es;
	R.hdr = L.hdr;
	R.desc = L.desc;
	R.out = po_d;
	R.out_next = Z.out_next;
	R.cm_out = L.cm;
	R.comp = c0->dev;
	R.delta = prot ? (int32_t)grow : -(int32_t)grow;
	err = sgpu_run_rpplan(d->arena, d->arena_size, &R, stream);
	if (err) {
		w->fz_d = NULL;
		return err;
	}
	w->fz_par ^= 1;
	/* CTR: the lean kernel's SRTCP form (srtp_gpu_tune nolean: the
	 * general compact kernel) */
	C = compact_of(d, &L);
	C.nfail = &po_d->nfail;
	C.uniform = gcm || g_env.nolean ? 1 : 4;
	C.guard = &po_d->fail;
	C.rtcp = 1;
	err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
			       (int)c0->nr, gcm ? 0 : 2, prot, stream);
	if (!err)   /* the results, guarded by the plan */
		err = sgpu_plan_results(&po_d->fail, R.es, d->end, d->err,
					(uint32_t)n, R.delta, stream);
	if (!err)
		err = g_env.nopost ? sgpu_memcpy_d2h(po, po_d, sizeof(*po), stream)
				   : sgpu_plan_post(po_d, po, sizeof(*po), NULL,
						    NULL, 0, stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return err;
	if (po->fail && g_env.times)
		fprintf(stderr, "re_srtp rtcp plan n=%zu %s: rejected "
			"(SPF %#x)\n", n, prot ? "protect" : "unprotect",
			po->fail);
	return rplanned_done(s, d, po, prot, C, L.es, pfail);
}

/*
 * Single-stream SRTCP batch planned and processed on the device (the
 * SRTCP counterpart of dev_planned): by default the one-launch plan above;
 * srtp_gpu_tune noplanfuse: k_parse (with the E || index words),
 * k_plan_rtcp, the compact crypto launch, the per-packet results; one host
 * synchronisation.  -1: not plannable or a forged packet (undone), else 0
 * / errno.
 */
int dev_planned_rtcp(int op, struct srtp *s, struct srtp_batch_dev *d,
		     uint32_t *pfail)
{
	*pfail = 0;
	if (!g_env.noplanfuse)
		return dev_lplanned_rtcp(op, s, d, pfail);
	const int prot = op == OP_RTCP_ENC;
	const struct comp *c0 = &s->rtcp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const uint32_t T = c0->tag_len;             /* 0 for GCM */
	const uint32_t grow = 4u + T + (gcm ? 16u : 0u);
	/* hd: the parsed headers | the E || index words */
	const struct ws_sizes z = {
		.hd = n * (sizeof(struct sgpu_hdr) + 12), .dsc = n * 12,
		.vs = n * 5 + 64, .cm = 4,
		.pl = sizeof(struct sgpu_plan_out) + 64, .es = n * 4};
	struct ws_layout L;
	struct sgpu_compact C;
	struct sgpu_rplan_in in;
	struct sgpu_plan_out *po, *po_d;
	uint32_t *eix_d;
	void *stream = d->stream;
	struct ws *w = ws_get();
	int err;

	if (!w)
		return ENOMEM;
	err = ws_layout_reserve(w, n, &z, &L);
	if (err)
		return err;
	eix_d = (uint32_t *)(w->hd.d + n * sizeof(struct sgpu_hdr));
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;

	rplan_in(&in, s, (uint32_t)n, prot);
	{
		/* parse (+ E || index words) + end copy + zeroed counters and
		 * plan + comp map, one launch */
		struct sgpu_prologue pro = {
			.end_copy = L.es, .z0 = L.nfail, .z1 = (uint32_t *)po_d,
			.nz0 = 1, .nz1 = (uint32_t)(sizeof(*po) / 4),
			.cm_out = L.cm, .cm = c0->dev};
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, L.hdr, prot ? NULL : eix_d,
					  (uint32_t)n, 1, &pro, stream);
	}
	if (!err)
		err = sgpu_plan_rtcp(&in, L.hdr, eix_d, d->pos, L.es, d->cap,
				     d->arena_size, L.desc, po_d, stream);
	/* CTR: the lean kernel's SRTCP form (srtp_gpu_tune nolean: the
	 * general compact kernel) */
	C = compact_of(d, &L);
	C.uniform = gcm || g_env.nolean ? 1 : 4;
	C.guard = gcm ? &po_d->fail : &po_d->skip[2];
	C.rtcp = 1;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : 2, prot, stream);
	if (!err)
		err = sgpu_plan_finish(&po_d->fail, L.es, d->end, d->err,
				       (uint32_t)n,
				       prot ? (int32_t)grow : -(int32_t)grow,
				       L.nfail, NULL, &po_d->nfail, NULL, stream);
	if (!err)
		err = sgpu_memcpy_d2h(po, po_d, sizeof(*po), stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return err;
	return rplanned_done(s, d, po, prot, C, L.es, pfail);
}

/* ---- SRTCP, one session, several SSRCs or disturbed arrivals ------------ */
/* (plan_streams_rtcp.hip) */

/* a rejected one-stream SRTCP plan the per-stream planner may take: only a
 * second SSRC (or one other than the known stream's) or a replayed or
 * decreasing index was in its way */
int srp_eligible(uint32_t pfail)
{
	return !g_env.nosrplan && pfail &&
	       !(pfail & ~(uint32_t)(SPF_SSRC | SPF_REPLAY));
}

/*
 * One-session SRTCP protect / unprotect batch over up to SRTP_MAX_STREAMS
 * SSRCs in any arrival order: the RTCP parse prologue (with the E || index
 * words for unprotect), sgpu_splan_rtcp, the general descriptor-driven crypto
 * launch (class 2, GCM 0) guarded by its verdict, the guarded results, one
 * copy back, one synchronisation; then the streams the batch opened are
 * appended in first-appearance order and every touched stream takes its
 * rtcp_index (protect) or replay window (unprotect, HMAC suites) after the
 * batch.  0: done; -1: declined (a 9th SSRC, a copy older than the look-back,
 * any other failed check, an imported window beyond 31 bits), or a forged
 * packet (undone) -- nothing modified, nothing counted but srundos, the
 * caller's fallback continues; errno.
 */
int dev_splanned_rtcp(int op, struct srtp *s, struct srtp_batch_dev *d)
{
	const int prot = op == OP_RTCP_ENC;
	const struct comp *c0 = &s->rtcp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const int rxh = !prot && c0->has_hmac;
	const size_t n = d->n;
	const uint32_t grow = 4u + c0->tag_len + (gcm ? 16u : 0u);
	const int32_t delta = prot ? (int32_t)grow : -(int32_t)grow;
	const size_t scr = sgpu_splan_rtcp_scratch((uint32_t)n);
	/* hd: the parsed headers | the E || index words */
	const struct ws_sizes z = {
		.hd = n * (sizeof(struct sgpu_hdr) + 12), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4,
		.pl = 64 + sizeof(struct sgpu_srplan_out), .es = n * 4};
	struct ws_layout L;
	struct sgpu_compact C;
	struct sgpu_srplan_in in;
	struct sgpu_srplan_out *ro, *ro_d;
	uint32_t *eix_d;
	void *stream = d->stream;
	struct ws *w = ws_get();
	unsigned k, nst;
	int err;

	if (!w)
		return ENOMEM;
	if (s->nstreams > SRTP_MAX_STREAMS)
		return -1;
	/* the records hold 32 bits of the window's top (an imported one may
	 * lie higher: the host's replay_check takes it) */
	if (rxh)
		for (k = 0; k < s->nstreams; k++)
			if (s->streams[k].replay_rtcp.lix > 0x7fffffffu)
				return -1;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = pool_reserve(w, &w->mscr, scr);
	if (err)
		return err;
	eix_d = (uint32_t *)(w->hd.d + n * sizeof(struct sgpu_hdr));
	ro = (struct sgpu_srplan_out *)w->pl.h;
	ro_d = (struct sgpu_srplan_out *)w->pl.d;

	memset(&in, 0, sizeof(in));
	rplan_in(&in.c, s, (uint32_t)n, prot);
	in.nst = s->nstreams;
	in.lookback = RX_LOOKBACK;
	in.zeroed = 1;
	for (k = 0; k < s->nstreams; k++) {
		const struct srtp_stream *x = &s->streams[k];
		in.st[k].ssrc = x->ssrc;
		in.st[k].ix = prot ? x->rtcp_index : (uint32_t)x->replay_rtcp.lix;
		in.st[k].blo = (uint32_t)x->replay_rtcp.bitmap;
		in.st[k].bhi = (uint32_t)(x->replay_rtcp.bitmap >> 32);
	}
	{
		/* one launch: parse (+ E || index words) + end copy + zeroed
		 * plan out + comp map */
		struct sgpu_prologue pro = {
			.end_copy = L.es, .z0 = (uint32_t *)ro_d,
			.nz0 = (uint32_t)(sizeof(*ro) / 4), .cm_out = L.cm,
			.cm = c0->dev};
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, L.hdr, prot ? NULL : eix_d,
					  (uint32_t)n, 1, &pro, stream);
	}
	if (!err)
		err = sgpu_splan_rtcp(&in, L.hdr, prot ? NULL : eix_d, d->pos,
				      L.es, d->cap, d->arena_size, L.desc,
				      w->mscr.d, scr, ro_d, stream);
	/* the general kernel's SRTCP form: E per packet from desc (an
	 * EALREADY packet: MAC only) */
	C = compact_of(d, &L);
	C.nfail = &ro_d->tab.base.nfail;
	C.uniform = 1;
	C.guard = &ro_d->tab.base.fail;
	C.rtcp = 1;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : 2, prot, stream);
	if (!err)
		err = sgpu_splan_rtcp_commit(&in, ro_d, w->mscr.d, L.es, d->end,
					     d->err, delta, stream);
	if (!err)
		err = sgpu_memcpy_d2h(ro, ro_d, sizeof(*ro), stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return err;
	if (ro->tab.base.fail) {
		if (g_env.times)
			fprintf(stderr, "re_srtp rtcp streams plan n=%zu %s: "
				"declined (SPF %#x)\n", n,
				prot ? "protect" : "unprotect", ro->tab.base.fail);
		return -1;
	}
	if (ro->tab.base.nfail) {
		/* a forged packet: undo on the device (the results were not
		 * written), fold on the host engine -- which counts the misses
		 * and the one fold, as it does without this planner */
		count(&g_cnt_srundos, 1);
		return undo_synced(undo_rtcp(d, C, c0), stream);
	}
	/* every touched stream's state after the batch */
	nst = streams_append(s, &ro->tab);
	for (k = 0; k < nst; k++) {
		struct srtp_stream *x = &s->streams[k];
		const struct sgpu_rtcp_rec *a = &ro->after[k];
		if (!ro->cnt[k])
			continue;
		if (prot) {
			x->rtcp_index = a->ix;
		}
		else if (rxh) {
			x->replay_rtcp.lix = a->ix;
			x->replay_rtcp.bitmap = (uint64_t)a->bhi << 32 | a->blo;
		}
	}
	count(&g_cnt_srplans, 1);
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	return 0;
}

/* ---- many sessions: what the bucket planners' routes share ------------- */

_Static_assert(sizeof(struct sgpu_sstate) == BP_SSTATE,
	       "bp_layout.h: sout holds one struct sgpu_sstate per session");

/* w->pl of these routes: plan out | fold out (the scatter zeroes its fail
 * word; only the resident in-order route folds) | the receive routes'
 * sgpu_bprx_out */
#define PL_FOFF ((sizeof(struct sgpu_plan_out) + 63) & ~(size_t)63)

/* bucket geometry (sgpu_bplan_geometry: -1, the buckets do not take the
 * batch) */
struct bgeo {
	uint32_t bshift, nb, cap;
};

static int bgeo_get(size_t n, size_t nsess, struct bgeo *g)
{
	return sgpu_bplan_geometry((uint32_t)n, (uint32_t)nsess, &g->bshift,
				   &g->nb, &g->cap);
}

/* a call's regions of w->bp on the device (NULL: not among its parts) */
struct bp_ptrs {
	void *ticket, *obins, *bcount;
	void *tmp, *sorted, *afail, *sseg, *sout, *order, *cnt, *rs;
};

/* reserve w->bp as bp_layout.h cuts it up for the call, zero the head of a
 * new pool (or of one a call did not finish on: w->bp_d) and hand out the
 * call's regions; 0 / errno */
static int bp_take(struct ws *w, size_t n, size_t nsess, const struct bgeo *g,
		   enum bp_parts parts, void *stream, struct bp_ptrs *P)
{
	const struct bp_layout l = bp_layout(n, nsess, g->nb, g->cap, parts);
	uint8_t *p;
	int err = pool_reserve(w, &w->bp, l.total);

	if (err)
		return err;
	p = w->bp.d;
	if (w->bp_d != p) {
		err = sgpu_memset(p, 0, BP_HEAD, stream);
		if (err)
			return err;
		w->bp_d = p;
	}
#define BP_AT(f) .f = l.f ? p + l.f : NULL
	*P = (struct bp_ptrs){
		.ticket = p + l.ticket, .obins = p + l.obins,
		.bcount = p + l.bcount, BP_AT(tmp), BP_AT(sorted), BP_AT(afail),
		BP_AT(sseg), BP_AT(sout), BP_AT(order), BP_AT(cnt), BP_AT(rs)};
#undef BP_AT
	return 0;
}

/* a bucket route's launches or its synchronisation failed: the stream
 * drained, so no copy still reads the host buffers, and the counters in
 * w->bp from zero next time */
static int bp_failed(int err, struct ws *w, void *stream)
{
	sgpu_stream_sync(stream);
	w->bp_d = NULL;
	return err;
}

/* what every RTP route fills alike of its bucket plan: the batch, the suite,
 * the geometry, the caller's arrays, the workspace layout, the call's regions
 * of w->bp, plan out and fold out in w->pl (pl_d); the rest zero */
static void bplan_fill(struct sgpu_bplan *B, int prot, const struct comp *c0,
		       const struct srtp_batch_dev *d, size_t nsess,
		       const struct ws_layout *L, const struct bgeo *g,
		       const struct bp_ptrs *P, uint8_t *pl_d)
{
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const uint32_t T = gcm ? 16u : c0->tag_len;

	*B = (struct sgpu_bplan){
		.n = (uint32_t)d->n, .nsess = (uint32_t)nsess,
		.prot = (uint32_t)prot, .tag = T,
		.need = prot ? (gcm ? 16u : (T > 4 ? T : 4u)) : 0u,
		.maxlen = SGPU_CACHED_MAX(c0->mode),
		.bshift = g->bshift, .nb = g->nb, .cap = g->cap,
		.delta = prot ? (int32_t)T : -(int32_t)T, .gcm = (uint32_t)gcm,
		.pos = d->pos, .end = d->end, .capv = d->cap, .sess = d->sess,
		.posw = d->pos, .endw = d->end, .err = d->err,
		.es = L->es, .hdr = L->hdr, .desc = L->desc, .nfail = L->nfail,
		.ticket = P->ticket, .obins = P->obins, .bcount = P->bcount,
		.tmp = P->tmp, .sorted = P->sorted, .afail = P->afail,
		.sseg = P->sseg, .sout = P->sout, .order = P->order,
		.out = (struct sgpu_plan_out *)pl_d,
		.fo = (struct sgpu_fold_out *)(pl_d + PL_FOFF)};
}

/* the same of an SRTCP bucket plan (s0: any of the batch's sessions, for
 * the suite) */
static void brtcp_fill(struct sgpu_bplan_rtcp *R, int prot,
		       const struct srtp *s0, const struct srtp_batch_dev *d,
		       size_t nsess, const struct ws_layout *L,
		       const struct bgeo *g, const struct bp_ptrs *P,
		       uint8_t *pl_d)
{
	const struct comp *c0 = &s0->rtcp;
	const uint32_t grow = 4u + c0->tag_len +
			      (c0->mode == SGPU_MODE_GCM ? 16u : 0u);

	*R = (struct sgpu_bplan_rtcp){
		.nsess = (uint32_t)nsess,
		.bshift = g->bshift, .nb = g->nb, .cap = g->cap,
		.delta = prot ? (int32_t)grow : -(int32_t)grow,
		.pos = d->pos, .end = d->end, .capv = d->cap, .sess = d->sess,
		.endw = d->end, .err = d->err,
		.es = L->es, .hdr = L->hdr, .desc = L->desc, .nfail = L->nfail,
		.bcount = P->bcount, .tmp = P->tmp, .afail = P->afail,
		.out = (struct sgpu_plan_out *)pl_d};
	/* the suite's part of the plan input; the streams come in the tables */
	rplan_in(&R->in, s0, (uint32_t)d->n, prot);
	R->in.ssrc_any = 0;
	R->in.ssrc = R->in.rtcp_index = 0;
	R->in.lix = R->in.bitmap = 0;
}

/*
 * The table routes plan against the host's stream tables: one upload in
 * w->ms (cm | toff | recs, the gathered part of it), one download of the
 * touched tables from w->mscr (sinfo | sout).  A receive route works on the
 * upload of the in-order route before it.
 */
struct tab_layout {
	size_t o_toff, o_recs;  /* in w->ms (cm: 0) */
	size_t up_max;          /* ... its bytes with every table full */
	size_t o_sout;          /* in w->mscr (sinfo: 0) */
	size_t down;            /* ... its bytes */
};

/* rec: bytes of a stream record (struct sgpu_rtp_rec / sgpu_rtcp_rec) */
static struct tab_layout tab_layout(size_t nsess, size_t rec)
{
	struct tab_layout t;
	t.o_toff = bp_al256(nsess * 4);
	t.o_recs = t.o_toff + bp_al256((nsess + 1) * 4);
	t.up_max = t.o_recs + nsess * SRTP_MAX_STREAMS * rec;
	t.o_sout = bp_al256(nsess * 4);
	t.down = t.o_sout + nsess * SRTP_MAX_STREAMS * rec;
	return t;
}

static int tab_reserve(struct ws *w, const struct tab_layout *t)
{
	int err = pool_reserve(w, &w->ms, t->up_max);
	if (!err)
		err = pool_reserve(w, &w->mscr, t->down);
	return err;
}

/* the upload must be the in-order route's: never a new pool */
static int tab_uploaded(const struct ws *w, const struct tab_layout *t)
{
	return w->ms.cap >= t->up_max && w->mscr.cap >= t->down;
}

/* ---- SRTCP, many sessions: forged packets settled on the device --------- */

/*
 * srtp_gpu_tune mrfold: a many-session SRTCP unprotect batch whose plan (R0:
 * dev_mplanned_rtcp's or dev_mrrxplanned's, as its scatter takes it) was
 * accepted and whose crypto launch C then counted nfail tag misses, behind
 * that call's synchronisation.  The verdict bytes of C are final, so nothing
 * is undone: HMAC suites run the scatter again, sgpu_bplan_rtcp_fold_settle
 * (the replay rule over the authentic arrivals alone), the keystream over the
 * packets the plan took for EALREADY and the settle accepts (C with undo = 1
 * and the settle's bytes for its verdicts), sgpu_bplan_rtcp_fold_finish, one
 * copy back of the touched tables; GCM suites, which keep no SRTCP replay
 * window, the results alone on the plan's own tables.  One synchronisation,
 * the apply (mrplan_apply).
 * 0: settled (misses += nfail, mrfolds +1); -1: the settle met a possible copy
 * older than the look-back -- the batch undone as without the knob, the host
 * engine folds (folds +1); errno.
 *
 * w->ms, w->mscr: struct tab_layout, as the plan left them; w->bp:
 * BP_TABLE_RX (bp_layout.h); w->pl: plan out | sgpu_bprx_out.
 */
static int mrfold_settle(struct srtp **sessv, size_t nsess,
			 struct srtp_batch_dev *d, struct ws *w,
			 const struct ws_layout *L, const struct bgeo *g,
			 const struct tab_layout *tab,
			 const struct sgpu_bplan_rtcp *R0, struct sgpu_compact C,
			 uint32_t nfail)
{
	const struct comp *c0 = &sessv[0]->rtcp;
	const size_t n = d->n;
	struct sgpu_plan_out *po = (struct sgpu_plan_out *)w->pl.h;
	struct sgpu_plan_out *po_d = (struct sgpu_plan_out *)w->pl.d;
	const struct sgpu_bprx_out *ro =
		(const struct sgpu_bprx_out *)(w->pl.h + PL_FOFF);
	struct sgpu_bplan_rtcp_fold F;
	struct sgpu_bplan_rtcp *R = &F.x.r;
	struct sgpu_compact K = C;
	struct bp_ptrs P;
	void *stream = d->stream;
	int err;

	memset(&F, 0, sizeof(F));
	F.vd = L->verdict;
	F.posw = d->pos;
	if (c0->mode == SGPU_MODE_GCM) {
		*R = *R0;
		err = sgpu_bplan_rtcp_fold_gcm(&F, stream);
		if (!err)
			err = sgpu_stream_sync(stream);
		if (err)
			return bp_failed(err, w, stream);
		goto settled;
	}
	if (w->pl.cap < PL_FOFF + sizeof(struct sgpu_bprx_out))
		return EINVAL;          /* (the routes reserve it: never) */
	err = bp_take(w, n, nsess, g, BP_TABLE_RX, stream, &P);
	if (err)
		return err;
	brtcp_fill(R, 0, sessv[0], d, nsess, L, g, &P, w->pl.d);
	R->toff = R0->toff;
	R->recs = R0->recs;
	R->sinfo = R0->sinfo;
	R->sout = R0->sout;
	R->outbytes = (uint32_t)(PL_FOFF + sizeof(struct sgpu_bprx_out));
	R->outh = g_env.nopost ? NULL : (uint32_t *)po;
	F.x.cnt = P.cnt;
	F.x.rs = P.rs;
	F.x.ro = (struct sgpu_bprx_out *)(w->pl.d + PL_FOFF);
	F.x.lookback = RX_LOOKBACK;
	{
		/* the scatter as the in-order plan launched it */
		struct sgpu_bplan_rtcp S = *R;
		S.outbytes = (uint32_t)offsetof(struct sgpu_plan_out, tail_ix);
		err = sgpu_bplan_rtcp_scatter(d->arena, d->arena_size, &S, stream);
	}
	if (!err)
		err = sgpu_bplan_rtcp_fold_settle(&F, stream);
	/* the keystream over the packets the settle names, guarded by it */
	K.undo = 1;
	K.verdict = P.rs;
	K.guard = &po_d->fail;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &K, c0->mode,
				       (int)c0->nr, 2, 0, stream);
	if (!err)
		err = sgpu_bplan_rtcp_fold_finish(&F, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(po, po_d, R->outbytes, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->mscr.h, w->mscr.d, tab->down, stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		/* declined: the packets, desc and the verdict bytes are as C left
		 * them (the keystream launch and the results did nothing); undo
		 * on the device, fold on the host engine */
		if (g_env.times)
			fprintf(stderr, "re_srtp mrfold n=%zu nsess=%zu: not "
				"settled (SPF %#x)\n", n, nsess, po->fail);
		count(&g_cnt_misses, nfail);
		count(&g_cnt_folds, 1);
		C.guard = NULL;         /* (the plan's: it held) */
		return undo_synced(undo_rtcp(d, C, c0), stream);
	}
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
settled:
	count(&g_cnt_misses, nfail);
	count(&g_cnt_mrfolds, 1);
	mrplan_apply(sessv, nsess, 0, (const uint32_t *)w->mscr.h,
		     (const struct sgpu_rtcp_rec *)(w->mscr.h + tab->o_sout));
	return 0;
}

/* ---- SRTCP, many sessions with up to 8 SSRCs each ---------------------- */

/*
 * An SRTCP protect / unprotect batch over many sessions, every array in
 * HBM, planned by the bucket planner of plan_buckets_rtcp.hip against the
 * host's stream tables (current: run_dev called sess_host; SRTCP state is
 * not resident).  One pass over the sessions gathers the tables
 * (mrplan_gather), one upload, sgpu_bplan_rtcp_scatter / _plan, the compact
 * crypto kernels with per-packet keys guarded by the plan, _finish, one copy
 * back of the touched tables, one synchronisation, the apply.  *pfail: a
 * rejected plan's SPF_* bits (0 otherwise).
 * 0: done; -1: a batch the geometry or the gather does not take (nothing
 * counted), a rejected plan, or a forged packet (undone) -- nothing
 * modified, the caller's fallback continues; errno.  With srtp_gpu_tune
 * mrfold an unprotect batch with forged packets goes to mrfold_settle.
 *
 * w->ms, w->mscr: struct tab_layout; w->bp: BP_TABLE (bp_layout.h).
 */
int dev_mplanned_rtcp(int op, struct srtp **sessv, size_t nsess,
		      struct srtp_batch_dev *d, uint32_t *pfail)
{
	const int prot = op == OP_RTCP_ENC;
	const struct comp *c0 = &sessv[0]->rtcp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const struct tab_layout tab =
		tab_layout(nsess, sizeof(struct sgpu_rtcp_rec));
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4,
		/* (mrfold: room for the settle's sgpu_bprx_out) */
		.pl = g_env.mrfold ? PL_FOFF + 64
				   : sizeof(struct sgpu_plan_out) + 64,
		.es = n * 4};
	struct ws_layout L;
	struct bgeo g;
	struct bp_ptrs P;
	struct sgpu_bplan_rtcp R;
	struct sgpu_compact C;
	struct sgpu_plan_out *po, *po_d;
	uint32_t *toff_h;
	size_t up;
	void *stream = d->stream;
	struct ws *w;
	const int times = g_env.times;
	double t[4];
	int err;

	*pfail = 0;
	if (bgeo_get(n, nsess, &g))
		return -1;
	w = ws_get();
	if (!w)
		return ENOMEM;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = tab_reserve(w, &tab);
	if (!err)
		err = bp_take(w, n, nsess, &g, BP_TABLE, stream, &P);
	if (err)
		return err;
	toff_h = (uint32_t *)(w->ms.h + tab.o_toff);
	t[0] = times ? now_ms() : 0;
	if (mrplan_gather(sessv, nsess, prot, toff_h,
			  (struct sgpu_rtcp_rec *)(w->ms.h + tab.o_recs),
			  (uint32_t *)w->ms.h))
		return -1;
	up = tab.o_recs + (size_t)toff_h[nsess] * sizeof(struct sgpu_rtcp_rec);
	t[1] = times ? now_ms() : 0;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	brtcp_fill(&R, prot, sessv[0], d, nsess, &L, &g, &P, w->pl.d);
	R.toff = (const uint32_t *)(w->ms.d + tab.o_toff);
	R.recs = (const struct sgpu_rtcp_rec *)(w->ms.d + tab.o_recs);
	R.sinfo = (uint32_t *)w->mscr.d;
	R.sout = (struct sgpu_rtcp_rec *)(w->mscr.d + tab.o_sout);
	R.outbytes = (uint32_t)offsetof(struct sgpu_plan_out, tail_ix);
	R.outh = g_env.nopost ? NULL : (uint32_t *)po;
	srv_stop(w);
	err = sgpu_memcpy_h2d(w->ms.d, w->ms.h, up, stream);
	if (!err)
		err = sgpu_bplan_rtcp_scatter(d->arena, d->arena_size, &R, stream);
	if (!err)
		err = sgpu_bplan_rtcp_plan(&R, stream);
	/* the compact kernels' SRTCP form with per-packet keys (AES-CM: class
	 * 2, the cipher region starts at byte 8), guarded by the plan */
	C = compact_of(d, &L);
	C.compmap = (const uint32_t *)w->ms.d;
	C.sess = d->sess;
	C.rtcp = 1;
	C.guard = &po_d->fail;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : 2, prot, stream);
	if (!err)
		err = sgpu_bplan_rtcp_finish(&R, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(po, po_d, R.outbytes, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->mscr.h, w->mscr.d, tab.down, stream);
	t[2] = times ? now_ms() : 0;
	if (!err)
		err = sgpu_stream_sync(stream);
	t[3] = times ? now_ms() : 0;
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		/* the crypto launch and the results did nothing */
		count(&g_cnt_rejects, 1);
		if (g_env.times)
			fprintf(stderr, "re_srtp mrtcp plan n=%zu nsess=%zu %s: "
				"rejected (SPF %#x)\n", n, nsess,
				prot ? "protect" : "unprotect", po->fail);
		*pfail = po->fail;
		return -1;
	}
	count(&g_cnt_mrplans, 1);
	if (po->nfail && g_env.mrfold && !prot && w->pl.cap >= PL_FOFF + 64)
		/* forged packets, settled on the device */
		return mrfold_settle(sessv, nsess, d, w, &L, &g, &tab, &R, C,
				     po->nfail);
	if (po->nfail) {
		/* a forged packet: undo on the device (no result was written,
		 * the host's tables are as they were), fold on the host engine */
		count(&g_cnt_misses, po->nfail);
		count(&g_cnt_folds, 1);
		return undo_synced(undo_rtcp(d, C, c0), stream);
	}
	mrplan_apply(sessv, nsess, prot, (const uint32_t *)w->mscr.h,
		     (const struct sgpu_rtcp_rec *)(w->mscr.h + tab.o_sout));
	if (times)
		fprintf(stderr, "re_srtp mrtcp plan n=%zu nsess=%zu %s: gather "
			"%.3f submit %.3f wait %.3f apply %.3f ms\n", n, nsess,
			prot ? "protect" : "unprotect", t[1] - t[0], t[2] - t[1],
			t[3] - t[2], now_ms() - t[3]);
	return 0;
}

/* ---- SRTCP, many sessions, reordered or replayed arrivals -------------- */

/* a rejected plan of dev_mplanned_rtcp the receive planner
 * (plan_buckets_rtcp_rx.hip) may settle: only an index that is not new and
 * increasing inside some stream was in its way (HMAC suites: GCM keeps no
 * SRTCP replay window and its plan takes any order) */
int mrrx_eligible(int op, const struct srtp *s, uint32_t pfail)
{
	return op == OP_RTCP_DEC && s->rtcp.has_hmac && !g_env.nomrplan &&
	       !g_env.nomrrxplan && pfail && !(pfail & ~(uint32_t)SPF_REPLAY);
}

/*
 * A many-session SRTCP unprotect batch behind such a rejection, on this
 * thread's workspace as dev_mplanned_rtcp left it: the rejected plan modified
 * nothing, so its upload (w->ms.d: cm | toff | recs) is still the truth and
 * nothing is gathered or uploaded again.  The bucket scatter again (the
 * rejected plan's finish zeroed its counters), sgpu_bplan_rtcp_rx_plan, the
 * compact crypto kernels with per-packet keys guarded by its verdict (an
 * EALREADY packet: MAC only), sgpu_bplan_rtcp_rx_finish, one copy back of the
 * touched tables, one synchronisation, the apply (mrplan_apply).
 * 0: done; -1: not settled, or a forged packet (undone) -- nothing modified,
 * the caller's fallback continues; errno.  With srtp_gpu_tune mrfold a batch
 * with forged packets goes to mrfold_settle.
 *
 * w->ms, w->mscr: struct tab_layout, as dev_mplanned_rtcp left them; w->bp:
 * BP_TABLE_RX (bp_layout.h); w->pl: plan out | sgpu_bprx_out.
 */
int dev_mrrxplanned(struct srtp **sessv, size_t nsess, struct srtp_batch_dev *d)
{
	const struct comp *c0 = &sessv[0]->rtcp;
	const size_t n = d->n;
	const struct tab_layout tab =
		tab_layout(nsess, sizeof(struct sgpu_rtcp_rec));
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4, .pl = PL_FOFF + 64, .es = n * 4};
	struct ws_layout L;
	struct bgeo g;
	struct bp_ptrs P;
	struct sgpu_bplan_rtcp_rx X;
	struct sgpu_bplan_rtcp *R = &X.r;
	struct sgpu_compact C;
	struct sgpu_plan_out *po, *po_d;
	const struct sgpu_bprx_out *ro;
	void *stream = d->stream;
	struct ws *w;
	int err;

	if (c0->mode == SGPU_MODE_GCM || !c0->has_hmac)
		return -1;
	if (bgeo_get(n, nsess, &g))
		return -1;
	w = ws_get();
	if (!w)
		return ENOMEM;
	if (!tab_uploaded(w, &tab))
		return -1;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = bp_take(w, n, nsess, &g, BP_TABLE_RX, stream, &P);
	if (err)
		return err;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	ro = (const struct sgpu_bprx_out *)(w->pl.h + PL_FOFF);
	memset(&X, 0, sizeof(X));
	brtcp_fill(R, 0, sessv[0], d, nsess, &L, &g, &P, w->pl.d);
	R->toff = (const uint32_t *)(w->ms.d + tab.o_toff);
	R->recs = (const struct sgpu_rtcp_rec *)(w->ms.d + tab.o_recs);
	R->sinfo = (uint32_t *)w->mscr.d;
	R->sout = (struct sgpu_rtcp_rec *)(w->mscr.d + tab.o_sout);
	R->outbytes = (uint32_t)(PL_FOFF + sizeof(struct sgpu_bprx_out));
	R->outh = g_env.nopost ? NULL : (uint32_t *)po;
	X.cnt = P.cnt;
	X.rs = P.rs;
	X.ro = (struct sgpu_bprx_out *)(w->pl.d + PL_FOFF);
	X.lookback = RX_LOOKBACK;
	srv_stop(w);
	{
		/* the scatter as the in-order plan launched it (it mirrors
		 * nothing: the plan out alone is its outbytes) */
		struct sgpu_bplan_rtcp S = *R;
		S.outbytes = (uint32_t)offsetof(struct sgpu_plan_out, tail_ix);
		err = sgpu_bplan_rtcp_scatter(d->arena, d->arena_size, &S, stream);
	}
	if (!err)
		err = sgpu_bplan_rtcp_rx_plan(&X, stream);
	/* the compact kernels' SRTCP form with per-packet keys (class 2),
	 * guarded by the plan */
	C = compact_of(d, &L);
	C.compmap = (const uint32_t *)w->ms.d;
	C.sess = d->sess;
	C.rtcp = 1;
	C.guard = &po_d->fail;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, 2, 0, stream);
	if (!err)
		err = sgpu_bplan_rtcp_rx_finish(&X, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(po, po_d, R->outbytes, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->mscr.h, w->mscr.d, tab.down, stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		/* the crypto launch and the results did nothing (the rejection
		 * was counted: dev_mplanned_rtcp's) */
		if (g_env.times)
			fprintf(stderr, "re_srtp mrrx plan n=%zu nsess=%zu: not "
				"settled (SPF %#x)\n", n, nsess, po->fail);
		return -1;
	}
	count(&g_cnt_mrrxplans, 1);
	if (po->nfail && g_env.mrfold)
		/* forged packets, settled on the device */
		return mrfold_settle(sessv, nsess, d, w, &L, &g, &tab, R, C,
				     po->nfail);
	if (po->nfail) {
		/* a forged packet: undo on the device (no result was written,
		 * the host's tables are as they were), fold on the host engine */
		count(&g_cnt_misses, po->nfail);
		count(&g_cnt_folds, 1);
		return undo_synced(undo_rtcp(d, C, c0), stream);
	}
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	mrplan_apply(sessv, nsess, 0, (const uint32_t *)w->mscr.h,
		     (const struct sgpu_rtcp_rec *)(w->mscr.h + tab.o_sout));
	return 0;
}

/*
 * Many sessions with at most one RTP stream each, every array in HBM: the
 * multi-session device planner (plan_multi.hip) plus the compact kernels
 * in length order, against the session states resident in HBM
 * (sgpu_sst_*); host work is one O(sessions) pass (slot map, residency).
 * The launches; -1: not plannable (after a synchronisation; nothing
 * modified).
 */
/* the multi-session verdict fold over the call's planner scratch (phase:
 * sgpu_mfold_rtp; nfail: the kernels' miss count, device, or NULL) */
static int mfold(struct dcall *k, int phase, const uint32_t *nfail,
		 const struct sgpu_sstate *sin_d, struct sgpu_sstate *sout_d,
		 size_t scr)
{
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const size_t n = d->n;
	struct sgpu_mplan_in in;
	struct ws_layout L;
	ws_layout_get(w, n, &L);
	memset(&in, 0, sizeof(in));
	in.n = (uint32_t)n;
	in.nsess = (uint32_t)k->nsess;
	return sgpu_mfold_rtp(phase, nfail, &in, L.hdr, d->sess, L.desc,
			      L.verdict, L.es, d->pos, d->end, d->err,
			      k->sessv[0]->rtp.mode == SGPU_MODE_GCM, sin_d,
			      sout_d, w->mscr.d, scr,
			      (uint32_t *)(w->pl.d + k->foff + 64),
			      (struct sgpu_fold_out *)(w->pl.d + k->foff),
			      d->stream);
}

/*
 * The bucket planner (plan_buckets.hip, srtpgpu.h struct sgpu_bplan): the
 * same plan, verdict fold and resident states as below, in three launches
 * around the crypto instead of ~17 plus the fold's five.
 *
 * w->bp: BP_RESIDENT (bp_layout.h); w->pl: plan out | fold out
 */
static int dev_bplanned_issue(struct dcall *k, const struct bgeo *g)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp **sessv = k->sessv;
	const size_t nsess = k->nsess;
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &sessv[0]->rtp;
	const size_t n = d->n;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	struct sgpu_bplan *B = &k->bp;
	struct bp_ptrs P;
	struct sgpu_sstate *up_h, *up_d;
	uint8_t *need_h, *need_d;
	uint32_t *cm_h;
	void *stream = d->stream;
	const int times = g_env.times;
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 9 + 72, .cm = nsess * 4, .pl = PL_FOFF + 64,
		.es = n * 4};
	struct ws_layout L;
	int err;

	k->foff = PL_FOFF;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)   /* uploads | need */
		err = pool_reserve(w, &w->ms,
				   nsess * (sizeof(struct sgpu_sstate) + 1));
	if (!err)
		err = bp_take(w, n, nsess, g, BP_RESIDENT, stream, &P);
	if (err)
		return err;
	bplan_fill(B, prot, c0, d, nsess, &L, g, &P, w->pl.d);
	k->devfold = !prot && !g_env.nodevfold;
	B->nofold = (uint32_t)!k->devfold;
	B->sst = sgpu_sst_table();
	B->pred = k->pred;
	B->gate = k->gate;
	B->verdict = L.verdict;
	B->flist = !prot && !gcm && k->devfold ? L.flist : NULL;
	/* parse, checks, bucket slots: no session state needed, so it runs
	 * while the host walks the sessions */
	err = sgpu_bplan_scatter(d->arena, d->arena_size, B, stream);
	if (err) {
		w->bp_d = NULL;
		return err;
	}
	cm_h = (uint32_t *)w->cm.h;
	up_h = (struct sgpu_sstate *)w->ms.h;
	need_h = (uint8_t *)(up_h + nsess);
	up_d = (struct sgpu_sstate *)w->ms.d;
	need_d = (uint8_t *)(up_d + nsess);
	k->t[0] = times ? now_ms() : 0;
	err = mplan_gather_res(sessv, nsess, up_h, cm_h, need_h, &k->nup,
			       k->pend, k->done);
	if (err) {
		/* the scatter only wrote scratch -- and the bucket counters,
		 * zeroed again before the workspace's next call */
		if (err == -2)
			k->pfail = MPF_MULTI;
		w->bp_d = NULL;
		err = sgpu_stream_sync(stream);
		return err ? err : -1;
	}
	k->t[1] = times ? now_ms() : 0;
	/* the slot map and the states the device lacks go up on the
	 * workspace's own stream (overlapping the kernels queued before on the
	 * call's stream); the call's stream waits for them before the plan */
	if (!w->upev)
		w->upev = sgpu_event_create();
	if (!w->upev) {
		w->bp_d = NULL;
		sgpu_stream_sync(stream);
		return ENOMEM;
	}
	srv_stop(w);
	err = sgpu_memcpy_h2d(w->cm.d, cm_h, nsess * 4, w->stream);
	if (!err && k->nup)
		err = sgpu_memcpy_h2d(up_d, up_h,
				      nsess * (sizeof(struct sgpu_sstate) + 1),
				      w->stream);
	if (!err)
		err = sgpu_event_record(w->upev, w->stream);
	if (!err)
		err = sgpu_stream_wait(stream, w->upev);
	if (err) {
		/* no copy may still read the host buffers */
		sgpu_stream_sync(w->stream);
		w->bp_d = NULL;
		return err;
	}
	B->cm = (const uint32_t *)w->cm.d;
	B->upneed = k->nup ? need_d : NULL;
	B->up = up_d;
	err = sgpu_bplan_plan(B, stream);
	if (!err) {
		/* the crypto launches behind the plan's guards (the class
		 * guards skip[] and the fail word), in its order */
		struct sgpu_compact C = compact_of(d, &L);
		C.sess = d->sess;
		C.idx = B->order;
		C.flist = (uint32_t *)B->flist;
		C.gfail = &B->out->fail;
		err = run_classes(d->arena, d->arena_size, C, c0,
				  B->out, prot, stream);
	}
	/* plan out and fold out back in one piece: written by the finish
	 * launch itself (srtp_gpu_tune nopost: one copy behind it) */
	B->outbytes = (uint32_t)(k->foff + sizeof(struct sgpu_fold_out));
	B->outh = g_env.nopost ? NULL : (uint32_t *)w->pl.h;
	if (!err)
		err = sgpu_bplan_finish(B, stream);
	if (err) {
		w->bp_d = NULL;
		return err;
	}
	if (g_env.nopost)
		err = sgpu_memcpy_d2h(w->pl.h, w->pl.d, B->outbytes, stream);
	k->t[2] = times ? now_ms() : 0;
	return err;
}

int dev_mplanned_issue(struct dcall *k)
{
	{
		struct bgeo g;
		if (!k->radix && !g_env.mpradix && !g_env.nobucket &&
		    !bgeo_get(k->d.n, k->nsess, &g)) {
			k->bucket = 1;
			return dev_bplanned_issue(k, &g);
		}
		k->bucket = 0;
	}

	const int prot = k->op == OP_RTP_ENC;
	struct srtp **sessv = k->sessv;
	const size_t nsess = k->nsess;
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &sessv[0]->rtp;
	const size_t n = d->n;
	const uint32_t T = c0->mode == SGPU_MODE_GCM ? 16u : c0->tag_len;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	struct sgpu_plan_out *po, *po_d;
	struct sgpu_fold_out *fo_d;
	struct sgpu_sstate *up_h, *up_d, *sin_d, *sout_d;
	struct sgpu_mplan_in in;
	/* pl: plan out | fold out | fold scratch (multi-session fold) */
	const size_t foff = PL_FOFF;
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 12,
		.vs = n * 9 + 72, .cm = nsess * 4,
		.pl = foff + 64 + sgpu_mfold_scratch((uint32_t)n), .es = n * 4};
	struct ws_layout L;
	struct sgpu_hdr *hd_d;
	uint64_t *desc_d;
	uint32_t *es_d, *nfail_d, *cm_h, *order_d, bits = 1;
	uint8_t *need_h, *need_d;
	size_t scr;
	void *stream = d->stream;
	const int times = g_env.times;
	int err;

	while (bits < 32 && ((size_t)1 << bits) < nsess)
		bits++;
	scr = sgpu_mplan_scratch((uint32_t)n, (uint32_t)nsess);
	k->foff = foff;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = pool_reserve(w, &w->ms,
				   nsess * (3 * sizeof(struct sgpu_sstate) + 1));
	if (!err)   /* scratch, the launch order (n words), then the parse
		     * prologue's window-check words (one per 256 packets) */
		err = pool_reserve(w, &w->mscr, scr + n * 4 + (n / 256 + 1) * 4);
	if (err)
		return err;
	hd_d = L.hdr;
	desc_d = L.desc;
	nfail_d = L.nfail;
	es_d = L.es;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	cm_h = (uint32_t *)w->cm.h;
	/* ms: st_in | st_out | uploads | need (device; host: the uploads) */
	sin_d = (struct sgpu_sstate *)w->ms.d;
	sout_d = sin_d + nsess;
	up_d = sout_d + nsess;
	need_d = (uint8_t *)(up_d + nsess);
	up_h = (struct sgpu_sstate *)w->ms.h + 2 * nsess;
	need_h = (uint8_t *)(up_h + nsess);
	order_d = (uint32_t *)(w->mscr.d + scr);
	/* parse + end copy (the kernels keep reading the input windows) +
	 * zeroed miss counter + the planner's window checks, one launch */
	memset(&in, 0, sizeof(in));
	in.wchk = (const uint32_t *)(w->mscr.d + scr + n * 4);
	{
		/* zeroes the plan out too (k_mp_iota ORs into it) and the
		 * counting grouping's per-session counters */
		const int radix = k->radix || g_env.mpradix || nsess > 65536;
		struct sgpu_prologue pro = {
			.end_copy = es_d, .z0 = nfail_d, .z1 = (uint32_t *)po_d,
			.nz0 = 1, .nz1 = (uint32_t)(sizeof(*po) / 4),
			.wchk = (uint32_t *)in.wchk, .cap = d->cap,
			.prot = (uint32_t)prot, .tag = T,
			.need = prot ? (gcm ? 16u : (T > 4 ? T : 4u)) : 0u,
			.maxlen = SGPU_CACHED_MAX(c0->mode),
			.z2 = radix ? NULL :
			      sgpu_mplan_counters(w->mscr.d, (uint32_t)n,
						  (uint32_t)nsess),
			.nz2 = radix ? 0u :
			       sgpu_mplan_counter_words((uint32_t)nsess)};
		in.radix = (uint32_t)radix;
		in.cnt_zeroed = !radix;
		err = sgpu_parse_prologue(d->arena, d->arena_size, d->pos,
					  d->end, hd_d, NULL, (uint32_t)n, 0,
					  &pro, stream);
		if (err)
			return err;
	}
	in.n = (uint32_t)n;
	in.nsess = (uint32_t)nsess;
	in.prot = (uint32_t)prot;
	in.tag = T;
	in.need = prot ? (gcm ? 16u : (T > 4 ? T : 4u)) : 0u;
	in.maxlen = SGPU_CACHED_MAX(c0->mode);
	in.key_bits = bits;
	in.out_zeroed = 1;
	/* the sort by session needs no session state: it runs while the
	 * host walks the sessions */
	err = sgpu_mplan_rtp_phase(1, &in, hd_d, d->pos, es_d, d->cap,
				   d->arena_size, d->sess, sin_d, sout_d,
				   desc_d, w->mscr.d, scr, po_d, order_d,
				   stream);
	if (!err && k->pred)
		err = sgpu_gate_pred(k->pred, &po_d->fail, stream);
	if (err)
		return err;
	/* one pass over the sessions: suite check, slot map, and the states
	 * the device does not hold yet (none once sessions are resident) */
	k->t[0] = times ? now_ms() : 0;
	err = mplan_gather_res(sessv, nsess, up_h, cm_h, need_h, &k->nup,
			       k->pend, k->done);
	if (err) {
		/* the queued sort only wrote scratch */
		if (err == -2)
			k->pfail = MPF_MULTI;
		err = sgpu_stream_sync(stream);
		return err ? err : -1;
	}
	k->t[1] = times ? now_ms() : 0;
	/* the slot map and the states the device lacks (64K fresh sessions:
	 * 2 MB) go up on the workspace's own stream, so the copy overlaps
	 * the kernels queued before it on the call's stream (the sort above,
	 * or the previous call's crypto launch) instead of following them;
	 * the call's stream waits for it before k_sst_load.  Nothing queued
	 * before reads cm or the uploads, and the workspace is not reused
	 * before the call completes. */
	if (!w->upev)
		w->upev = sgpu_event_create();
	if (!w->upev)
		return ENOMEM;
	srv_stop(w);
	err = sgpu_memcpy_h2d(w->cm.d, cm_h, nsess * 4, w->stream);
	if (!err && k->nup)
		err = sgpu_memcpy_h2d(up_d, up_h,
				      nsess * (sizeof(struct sgpu_sstate) + 1),
				      w->stream);
	if (!err)
		err = sgpu_event_record(w->upev, w->stream);
	if (!err)
		err = sgpu_stream_wait(stream, w->upev);
	if (err) {
		/* no copy may still read the host buffers */
		sgpu_stream_sync(w->stream);
		return err;
	}
	if (!err)
		err = sgpu_sst_load((const uint32_t *)w->cm.d,
				    k->nup ? need_d : NULL, up_d,
				    (uint32_t)nsess, sin_d, stream);
	if (!err)
		err = sgpu_mplan_rtp_phase(2, &in, hd_d, d->pos, es_d, d->cap,
					   d->arena_size, d->sess, sin_d,
					   sout_d, desc_d, w->mscr.d, scr, po_d,
					   order_d, stream);
	if (!err) {
		/* unprotect (CTR): forged packets are listed and restored
		 * behind the kernel, for the device fold (dev_mplanned_finish) */
		struct sgpu_compact C = compact_of(d, &L);
		C.sess = d->sess;
		C.idx = order_d;
		C.flist = !prot && !gcm && !g_env.nodevfold ? L.flist : NULL;
		err = run_classes(d->arena, d->arena_size, C, c0,
				  po_d, prot, stream);
	}
	/* unprotect: the verdict fold queued behind the kernels (it does
	 * nothing without a miss), so a forged packet neither gates the next
	 * chained call nor waits for the host: srtp.c:310-321, 342-359,
	 * 426-427 per session segment (sgpu_mfold_rtp) */
	k->devfold = !prot && !g_env.nodevfold;
	fo_d = (struct sgpu_fold_out *)(w->pl.d + k->foff);
	if (!err && k->devfold)
		err = mfold(k, 1, nfail_d, sin_d, sout_d, scr);
	if (!err)
		err = sgpu_plan_finish(&po_d->fail, es_d, d->end, d->err,
				       (uint32_t)n,
				       prot ? (int32_t)T : -(int32_t)T, nfail_d,
				       k->gate, &po_d->nfail,
				       k->devfold ? &fo_d->fail : NULL, stream);
	if (!err && k->devfold)
		err = mfold(k, 2, nfail_d, sin_d, sout_d, scr);
	/* the new states replace the resident ones if the plan held and
	 * every tag verified or the fold held (else the host folds from the
	 * old ones) */
	if (!err)
		err = sgpu_sst_commit((const uint32_t *)w->cm.d, sout_d,
				      (uint32_t)nsess, &po_d->fail,
				      k->devfold ? &fo_d->fail : nfail_d, stream);
	/* plan out and fold out in one copy */
	if (!err)
		err = sgpu_memcpy_d2h(po, po_d, k->foff + sizeof(*fo_d), stream);
	k->t[2] = times ? now_ms() : 0;
	return err;
}

/* ... after its launches completed: 0 / errno, -1 not plannable or a
 * forged packet (undone; the host folds), -2 gated by the chained call
 * before (nothing modified) */
int dev_mplanned_finish(struct dcall *k)
{
	const int prot = k->op == OP_RTP_ENC;
	struct srtp **sessv = k->sessv;
	struct srtp_batch_dev *d = &k->d;
	struct ws *w = k->w;
	const struct comp *c0 = &sessv[0]->rtp;
	const size_t n = d->n;
	struct sgpu_plan_out *po = (struct sgpu_plan_out *)w->pl.h;
	struct sgpu_plan_out *po_d = (struct sgpu_plan_out *)w->pl.d;
	uint32_t nfail = po->nfail;
	struct ws_layout L;
	struct sgpu_compact C;

	k->pfail = po->fail;
	if (g_env.times)
		fprintf(stderr, "re_srtp mplan n=%zu nsess=%zu up=%u: gather "
			"%.3f submit %.3f wait %.3f ms\n", n, k->nsess, k->nup,
			k->t[1] - k->t[0], k->t[2] - k->t[1],
			now_ms() - k->t[2]);
	if (po->fail) {
		if (po->fail & SPF_PRED)
			return -2;
		count(&g_cnt_rejects, 1);
		return -1;
	}
	count(&g_cnt_mplans, 1);
	if (!nfail)
		return 0;
	count(&g_cnt_misses, nfail);
	/* a forged packet: fold the verdicts on the device, per session
	 * (sgpu_mfold_rtp).  The kernels left each forged packet as
	 * srtp_decrypt does (HMAC: ciphertext restored, the ROC over the tag;
	 * GCM: decrypted in place); the fold checks the speculation under the
	 * true s_l and writes the EAUTH results and the touched sessions'
	 * states, which then replace the resident ones. */
	if (!prot && k->devfold) {
		/* folded on the device behind the kernels (dev_mplanned_issue);
		 * its verdict came back with the plan */
		const struct sgpu_fold_out *fo =
			(const struct sgpu_fold_out *)(w->pl.h + k->foff);
		if (!fo->fail) {
			count(&g_cnt_devfolds, 1);
			return 0;
		}
	}
	count(&g_cnt_folds, 1);
	/* undo on the device, fold on the host engine (the resident states
	 * are untouched) */
	ws_layout_get(w, n, &L);
	C = compact_of(d, &L);
	C.sess = d->sess;
	C.undo = 1;
	return undone(run_classes(d->arena, d->arena_size, C, c0, po_d, prot,
				  d->stream), d, L.es);
}

/* synchronous: -1 not plannable (nothing modified), else 0 / errno */
int dev_mplanned_(int op, struct srtp **sessv, size_t nsess,
			 struct srtp_batch_dev *d, int radix, uint32_t *pfail)
{
	return dev_call(op, sessv, nsess, d, radix, dev_mplanned_issue,
			dev_mplanned_finish, 0, pfail);
}

/* a session with more than SGPU_MP_SEGMAX packets (SPF_SEG): re-planned
 * with the radix-sort grouping */
int dev_mplanned(int op, struct srtp **sessv, size_t nsess,
			struct srtp_batch_dev *d, uint32_t *pfail)
{
	uint32_t pf = 0;
	int r = dev_mplanned_(op, sessv, nsess, d, g_env.mpradix, &pf);
	if (r == -1 && (pf & SPF_SEG) && !g_env.mpradix)
		r = dev_mplanned_(op, sessv, nsess, d, 1, &pf);
	*pfail = pf;
	return r;
}

/* ---- many sessions, reordered / duplicated arrivals -------------------- */

/* a rejected many-session unprotect plan the bucket receive planner
 * (plan_buckets_rx.hip) may settle: the bucket planner produced it, and only
 * the arrival order or a replayed index inside some session was in its way
 * (a batch the buckets do not take: dev_mrxplanned's -1) */
int mrx_eligible(int op, size_t nsess, uint32_t pfail)
{
	return op == OP_RTP_DEC && nsess > 1 && !g_env.norxplan &&
	       !g_env.nobucket && !g_env.mpradix && pfail &&
	       !(pfail & ~(uint32_t)(SPF_ORDER | SPF_REPLAY));
}

/*
 * A many-session unprotect batch behind such a rejection, every array in
 * HBM, against the resident states: the bucket scatter again (the rejected
 * plan's finish zeroed its counters), the state gather of
 * dev_bplanned_issue, sgpu_bplan_rx_plan, the general descriptor-driven
 * crypto launches in array order guarded by its verdict, sgpu_bplan_rx_finish
 * (results and the commit of the touched states, only if every packet was
 * settled and every tag verified), one synchronisation.
 * 0: done, the states advanced on the device (the sessions stay resident,
 * as after dev_mplanned); -1: not settled, a batch the gather refuses, or a
 * forged packet (undone) -- nothing modified, the caller's fallback
 * continues; errno.
 *
 * w->bp: BP_RESIDENT_RX (bp_layout.h); w->pl: plan out | fold out (unused) |
 * sgpu_bprx_out.
 */
int dev_mrxplanned(struct srtp **sessv, size_t nsess, struct srtp_batch_dev *d)
{
	const struct comp *c0 = &sessv[0]->rtp;
	const size_t n = d->n;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = nsess * 4, .pl = PL_FOFF + 128,
		.es = n * 4};
	struct ws_layout L;
	struct bgeo g;
	struct bp_ptrs P;
	struct sgpu_bplan_rx R;
	struct sgpu_bplan *B = &R.b;
	struct sgpu_compact C;
	struct sgpu_plan_out *po, *po_d;
	const struct sgpu_bprx_out *ro;
	struct sgpu_sstate *up_h, *up_d;
	uint8_t *need_h, *need_d;
	uint32_t *cm_h, nup = 0;
	void *stream = d->stream;
	struct ws *w;
	int err;

	if (bgeo_get(n, nsess, &g))
		return -1;
	w = ws_get();
	if (!w)
		return ENOMEM;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)   /* uploads | need */
		err = pool_reserve(w, &w->ms,
				   nsess * (sizeof(struct sgpu_sstate) + 1));
	if (!err)
		err = bp_take(w, n, nsess, &g, BP_RESIDENT_RX, stream, &P);
	if (err)
		return err;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	ro = (const struct sgpu_bprx_out *)(w->pl.h + PL_FOFF + 64);
	memset(&R, 0, sizeof(R));
	bplan_fill(B, 0, c0, d, nsess, &L, &g, &P, w->pl.d);
	B->sst = sgpu_sst_table();
	B->verdict = L.verdict;
	R.cnt = P.cnt;
	R.rs = P.rs;
	R.ro = (struct sgpu_bprx_out *)(w->pl.d + PL_FOFF + 64);
	R.lookback = RX_LOOKBACK;
	R.hmac = !gcm;
	err = sgpu_bplan_scatter(d->arena, d->arena_size, B, stream);
	if (err) {
		w->bp_d = NULL;
		return err;
	}
	cm_h = (uint32_t *)w->cm.h;
	up_h = (struct sgpu_sstate *)w->ms.h;
	need_h = (uint8_t *)(up_h + nsess);
	up_d = (struct sgpu_sstate *)w->ms.d;
	need_d = (uint8_t *)(up_d + nsess);
	if (mplan_gather_res(sessv, nsess, up_h, cm_h, need_h, &nup, 0, 0)) {
		/* the scatter only wrote scratch -- and the bucket counters,
		 * zeroed again before the workspace's next call */
		w->bp_d = NULL;
		err = sgpu_stream_sync(stream);
		return err ? err : -1;
	}
	/* the slot map (and any state the device lacks: none behind a bucket
	 * plan that just uploaded them) on the call's stream */
	err = sgpu_memcpy_h2d(w->cm.d, cm_h, nsess * 4, stream);
	if (!err && nup)
		err = sgpu_memcpy_h2d(up_d, up_h,
				      nsess * (sizeof(struct sgpu_sstate) + 1),
				      stream);
	B->cm = (const uint32_t *)w->cm.d;
	B->upneed = nup ? need_d : NULL;
	B->up = up_d;
	if (!err)
		err = sgpu_bplan_rx_plan(&R, stream);
	/* the general kernels (EALREADY packets: MAC only) with per-packet
	 * session keys, array order: AES-CM picks the header class from
	 * skip[], GCM has one */
	C = compact_of(d, &L);
	C.sess = d->sess;
	C.guard = gcm ? &po_d->fail : po_d->skip;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : -1, 0, stream);
	B->outbytes = (uint32_t)(PL_FOFF + 64 + sizeof(struct sgpu_bprx_out));
	B->outh = g_env.nopost ? NULL : (uint32_t *)w->pl.h;
	if (!err)
		err = sgpu_bplan_rx_finish(&R, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(w->pl.h, w->pl.d, B->outbytes, stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		if (g_env.times)
			fprintf(stderr, "re_srtp mrx plan n=%zu nsess=%zu: not "
				"settled (SPF %#x)\n", n, nsess, po->fail);
		return -1;
	}
	if (po->nfail) {
		/* a forged packet: undo on the device (no result and no state
		 * was written), fold on the host engine */
		count(&g_cnt_misses, po->nfail);
		count(&g_cnt_folds, 1);
		C.undo = 1;
		return undo_synced(run_classes(d->arena, d->arena_size, C, c0,
					       po_d, 0, stream), stream);
	}
	count(&g_cnt_mrxplans, 1);
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	return 0;
}

/* ---- many sessions with up to 8 SSRCs each, in order ------------------- */

/* a many-session RTP batch the bucket planner left for the planner of
 * plan_buckets_rtp_streams.hip: its gather met a session that holds several
 * streams (MPF_MULTI: no plan was tried), or its plan came back rejected for
 * a second SSRC inside some session -- beside which a rejection for the
 * order or a replayed index may only be that of two streams read as one */
int ms_eligible(int op, size_t nsess, uint32_t pfail)
{
	if ((op != OP_RTP_ENC && op != OP_RTP_DEC) || nsess < 2 ||
	    g_env.nomsplan)
		return 0;
	if (pfail == MPF_MULTI)
		return 1;
	return (pfail & SPF_SSRC) &&
	       !(pfail & ~(uint32_t)(SPF_SSRC | SPF_ORDER | SPF_REPLAY));
}

/*
 * Such a batch, every array in HBM, planned against the host's stream
 * tables (current: run_dev called sess_host; the tables of sessions with
 * several streams are not resident).  One pass over the sessions gathers the
 * tables (msplan_gather), one upload, the bucket scatter (again: a rejected
 * bucket plan's finish zeroed its counters), sgpu_bplan_rtps_plan, the
 * general descriptor-driven crypto kernels with per-packet keys guarded by
 * the plan, sgpu_bplan_rtps_finish, one copy back of the touched tables, one
 * synchronisation, the apply.  counted: a plan of this call was counted as
 * rejected already (rejects moves at most once per call); *pfail: a rejected
 * plan's SPF_* bits (0 otherwise).
 * 0: done; -1: a batch the geometry or the gather does not take (nothing
 * counted), a rejected plan, or a forged packet (undone) -- nothing
 * modified, the caller's fallback continues; errno.
 *
 * w->ms, w->mscr: struct tab_layout; w->bp: BP_TABLE (bp_layout.h), what the
 * scatter uses; w->pl: plan out | fold out (not used).
 */
int dev_msplanned(int op, struct srtp **sessv, size_t nsess,
		  struct srtp_batch_dev *d, int counted, uint32_t *pfail)
{
	const int prot = op == OP_RTP_ENC;
	const struct comp *c0 = &sessv[0]->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const struct tab_layout tab =
		tab_layout(nsess, sizeof(struct sgpu_rtp_rec));
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4, .pl = PL_FOFF + 64, .es = n * 4};
	struct ws_layout L;
	struct bgeo g;
	struct bp_ptrs P;
	struct sgpu_bplan_rtps R;
	struct sgpu_bplan *B = &R.b;
	struct sgpu_compact C;
	struct sgpu_plan_out *po, *po_d;
	uint32_t *toff_h;
	size_t up;
	void *stream = d->stream;
	struct ws *w;
	const int times = g_env.times;
	double t[4];
	int err;

	*pfail = 0;
	if (bgeo_get(n, nsess, &g))
		return -1;
	w = ws_get();
	if (!w)
		return ENOMEM;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = tab_reserve(w, &tab);
	if (!err)
		err = bp_take(w, n, nsess, &g, BP_TABLE, stream, &P);
	if (err)
		return err;
	toff_h = (uint32_t *)(w->ms.h + tab.o_toff);
	t[0] = times ? now_ms() : 0;
	if (msplan_gather(sessv, nsess, toff_h,
			  (struct sgpu_rtp_rec *)(w->ms.h + tab.o_recs),
			  (uint32_t *)w->ms.h))
		return -1;
	up = tab.o_recs + (size_t)toff_h[nsess] * sizeof(struct sgpu_rtp_rec);
	t[1] = times ? now_ms() : 0;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	memset(&R, 0, sizeof(R));
	bplan_fill(B, prot, c0, d, nsess, &L, &g, &P, w->pl.d);
	B->cm = (const uint32_t *)w->ms.d;
	B->outbytes = (uint32_t)offsetof(struct sgpu_plan_out, tail_ix);
	B->outh = g_env.nopost ? NULL : (uint32_t *)po;
	R.toff = (const uint32_t *)(w->ms.d + tab.o_toff);
	R.recs = (const struct sgpu_rtp_rec *)(w->ms.d + tab.o_recs);
	R.sinfo = (uint32_t *)w->mscr.d;
	R.sout = (struct sgpu_rtp_rec *)(w->mscr.d + tab.o_sout);
	srv_stop(w);
	err = sgpu_memcpy_h2d(w->ms.d, w->ms.h, up, stream);
	if (!err)
		err = sgpu_bplan_scatter(d->arena, d->arena_size, B, stream);
	if (!err)
		err = sgpu_bplan_rtps_plan(&R, stream);
	/* the general kernels with per-packet session keys, array order:
	 * AES-CM picks the header class from skip[], GCM has one */
	C = compact_of(d, &L);
	C.compmap = (const uint32_t *)w->ms.d;
	C.sess = d->sess;
	C.guard = gcm ? &po_d->fail : po_d->skip;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : -1, prot, stream);
	if (!err)
		err = sgpu_bplan_rtps_finish(&R, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(po, po_d, B->outbytes, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->mscr.h, w->mscr.d, tab.down, stream);
	t[2] = times ? now_ms() : 0;
	if (!err)
		err = sgpu_stream_sync(stream);
	t[3] = times ? now_ms() : 0;
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		/* the crypto launch and the results did nothing */
		if (!counted)
			count(&g_cnt_rejects, 1);
		if (g_env.times)
			fprintf(stderr, "re_srtp msplan n=%zu nsess=%zu %s: "
				"rejected (SPF %#x)\n", n, nsess,
				prot ? "protect" : "unprotect", po->fail);
		*pfail = po->fail;
		return -1;
	}
	if (po->nfail) {
		/* a forged packet: undo on the device (no result was written,
		 * the host's tables are as they were), fold on the host engine */
		count(&g_cnt_misses, po->nfail);
		count(&g_cnt_folds, 1);
		C.undo = 1;
		return undo_synced(run_classes(d->arena, d->arena_size, C, c0,
					       po_d, 0, stream), stream);
	}
	count(&g_cnt_msplans, 1);
	msplan_apply(sessv, nsess, prot, (const uint32_t *)w->mscr.h,
		     (const struct sgpu_rtp_rec *)(w->mscr.h + tab.o_sout));
	if (times)
		fprintf(stderr, "re_srtp msplan n=%zu nsess=%zu %s: gather "
			"%.3f submit %.3f wait %.3f apply %.3f ms\n", n, nsess,
			prot ? "protect" : "unprotect", t[1] - t[0], t[2] - t[1],
			t[3] - t[2], now_ms() - t[3]);
	return 0;
}

/* ---- many sessions with up to 8 SSRCs each, reordered arrivals --------- */

/* a rejected plan of dev_msplanned the receive planner
 * (plan_buckets_rtp_streams_rx.hip) may settle: only the arrival order or a
 * replayed index inside some stream was in its way */
int msrx_eligible(int op, uint32_t pfail)
{
	return op == OP_RTP_DEC && !g_env.nomsplan && !g_env.nomsrxplan &&
	       pfail && !(pfail & ~(uint32_t)(SPF_ORDER | SPF_REPLAY));
}

/*
 * A many-session unprotect batch behind such a rejection, on this thread's
 * workspace as dev_msplanned left it: the rejected plan modified nothing, so
 * its upload (w->ms.d: cm | toff | recs) is still the truth and nothing is
 * gathered or uploaded again.  The bucket scatter again (the rejected plan's
 * finish zeroed its counters), sgpu_bplan_rtps_rx_plan, the general
 * descriptor-driven crypto kernels in array order with per-packet keys
 * guarded by its verdict, sgpu_bplan_rtps_rx_finish, one copy back of the
 * touched tables, one synchronisation, the apply (msplan_apply).
 * 0: done; -1: not settled, or a forged packet (undone) -- nothing modified,
 * the caller's fallback continues; errno.
 *
 * w->ms, w->mscr: struct tab_layout, as dev_msplanned left them; w->bp:
 * BP_TABLE_RX (bp_layout.h); w->pl: plan out | fold out (unused) |
 * sgpu_bprx_out.
 */
int dev_msrxplanned(struct srtp **sessv, size_t nsess, struct srtp_batch_dev *d)
{
	const struct comp *c0 = &sessv[0]->rtp;
	const int gcm = c0->mode == SGPU_MODE_GCM;
	const size_t n = d->n;
	const struct tab_layout tab =
		tab_layout(nsess, sizeof(struct sgpu_rtp_rec));
	const struct ws_sizes z = {
		.hd = n * sizeof(struct sgpu_hdr), .dsc = n * 8,
		.vs = n * 5 + 64, .cm = 4, .pl = PL_FOFF + 128, .es = n * 4};
	struct ws_layout L;
	struct bgeo g;
	struct bp_ptrs P;
	struct sgpu_bplan_rtps_rx R;
	struct sgpu_bplan *B = &R.s.b;
	struct sgpu_compact C;
	struct sgpu_plan_out *po, *po_d;
	const struct sgpu_bprx_out *ro;
	void *stream = d->stream;
	struct ws *w;
	int err;

	if (bgeo_get(n, nsess, &g))
		return -1;
	w = ws_get();
	if (!w)
		return ENOMEM;
	if (!tab_uploaded(w, &tab))
		return -1;
	err = ws_layout_reserve(w, n, &z, &L);
	if (!err)
		err = bp_take(w, n, nsess, &g, BP_TABLE_RX, stream, &P);
	if (err)
		return err;
	po = (struct sgpu_plan_out *)w->pl.h;
	po_d = (struct sgpu_plan_out *)w->pl.d;
	ro = (const struct sgpu_bprx_out *)(w->pl.h + PL_FOFF + 64);
	memset(&R, 0, sizeof(R));
	bplan_fill(B, 0, c0, d, nsess, &L, &g, &P, w->pl.d);
	B->cm = (const uint32_t *)w->ms.d;
	B->outbytes = (uint32_t)(PL_FOFF + 64 + sizeof(struct sgpu_bprx_out));
	B->outh = g_env.nopost ? NULL : (uint32_t *)po;
	R.s.toff = (const uint32_t *)(w->ms.d + tab.o_toff);
	R.s.recs = (const struct sgpu_rtp_rec *)(w->ms.d + tab.o_recs);
	R.s.sinfo = (uint32_t *)w->mscr.d;
	R.s.sout = (struct sgpu_rtp_rec *)(w->mscr.d + tab.o_sout);
	R.cnt = P.cnt;
	R.rs = P.rs;
	R.ro = (struct sgpu_bprx_out *)(w->pl.d + PL_FOFF + 64);
	R.lookback = RX_LOOKBACK;
	R.hmac = !gcm;
	srv_stop(w);
	err = sgpu_bplan_scatter(d->arena, d->arena_size, B, stream);
	if (!err)
		err = sgpu_bplan_rtps_rx_plan(&R, stream);
	/* the general kernels (EALREADY packets: MAC only) with per-packet
	 * session keys, array order: AES-CM picks the header class from
	 * skip[], GCM has one */
	C = compact_of(d, &L);
	C.compmap = (const uint32_t *)w->ms.d;
	C.sess = d->sess;
	C.guard = gcm ? &po_d->fail : po_d->skip;
	if (!err)
		err = sgpu_run_compact(d->arena, d->arena_size, &C, c0->mode,
				       (int)c0->nr, gcm ? 0 : -1, 0, stream);
	if (!err)
		err = sgpu_bplan_rtps_rx_finish(&R, stream);
	if (!err && g_env.nopost)
		err = sgpu_memcpy_d2h(po, po_d, B->outbytes, stream);
	if (!err)
		err = sgpu_memcpy_d2h(w->mscr.h, w->mscr.d, tab.down, stream);
	if (!err)
		err = sgpu_stream_sync(stream);
	if (err)
		return bp_failed(err, w, stream);
	if (po->fail) {
		/* the crypto launch and the results did nothing (the rejection
		 * was counted: dev_msplanned's, or the bucket planner's) */
		if (g_env.times)
			fprintf(stderr, "re_srtp msrx plan n=%zu nsess=%zu: not "
				"settled (SPF %#x)\n", n, nsess, po->fail);
		return -1;
	}
	if (po->nfail) {
		/* a forged packet: undo on the device (no result was written,
		 * the host's tables are as they were), fold on the host engine */
		count(&g_cnt_misses, po->nfail);
		count(&g_cnt_folds, 1);
		C.undo = 1;
		return undo_synced(run_classes(d->arena, d->arena_size, C, c0,
					       po_d, 0, stream), stream);
	}
	count(&g_cnt_msrxplans, 1);
	count(&g_cnt_rxlate, ro->nlate);
	count(&g_cnt_rxdups, ro->ndup);
	msplan_apply(sessv, nsess, 0, (const uint32_t *)w->mscr.h,
		     (const struct sgpu_rtp_rec *)(w->mscr.h + tab.o_sout));
	return 0;
}
