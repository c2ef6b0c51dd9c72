/*
 * gen_roc_golden.c -- reference answers at large RTP rollover counters
 * (TEST INFRASTRUCTURE ONLY).
 *
 * Linked against the reference libre sources compiled by oracle/Makefile
 * (target `ref`), with the reference's private src/srtp/srtp.h so that a
 * stream can be put at any (roc, s_l, replay window), as srtp_stream_import
 * does in the product.  Streams start one packet-run below the boundaries
 * B = 2^16, 2^31 and 2^32 of the ROC and are driven across them:
 *
 *   tx_*   srtp_encrypt in order, all six suites
 *   rx_*   srtp_decrypt, suites 1 and 5: in order, swapped, late from before
 *          the boundary, duplicated on both sides, with a gap, the nine
 *          arrivals of DESIGN.md 5 -- each followed by a second batch that
 *          replays packets of the first beside new ones -- and a stream
 *          taken over at roc 0x80000005 with an empty window
 *
 * srtp_get_index (misc.c:22-41) holds the ROC in an int, so from 2^31 on the
 * index the replay window stores is sign-extended; behind 2^32 the ROC is 0
 * again while the window's top stays near 2^64.  Every call's input, output
 * bytes, errno, pos and end and the stream state after every batch are
 * recorded as JSON on stdout; no randomness, no time: two runs are identical.
 *
 * Usage: make -C oracle roc_golden
 *        (oracle/_ref/gen_roc_golden | gzip -9n >
 *         tests/golden/srtp_roc_golden.json.gz)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <re.h>
#include "srtp.h"               /* reference src/srtp/srtp.h (stream state) */

#define SSRC 0x524f4331u
#define NPKT 16                 /* packets the sender makes per case */
#define S_L0 65530u             /* s_l before the batch: seq 65531 is next */

static const struct {
	const char *name;
	uint32_t roc;           /* B - 1 */
} bounds[] = {
	{"2p16", 0x0000ffffu},
	{"2p31", 0x7fffffffu},
	{"2p32", 0xffffffffu},
};

static const size_t keylen[6] = {30, 30, 46, 46, 28, 44};

static void hexout(const uint8_t *p, size_t n)
{
	size_t i;
	putchar('"');
	for (i = 0; i < n; i++)
		printf("%02x", p[i]);
	putchar('"');
}

static void make_key(uint8_t *key, int suite, unsigned salt)
{
	size_t i;
	for (i = 0; i < keylen[suite]; i++)
		key[i] = (uint8_t)(29 * i + 7 * salt + 13 * suite + 1);
}

static struct srtp_stream *stream_at(struct srtp *s, uint32_t roc, uint16_t s_l,
				     int s_l_set, uint64_t lix, uint64_t bitmap)
{
	struct srtp_stream *st = NULL;
	if (stream_get(&st, s, SSRC)) {
		fprintf(stderr, "stream_get failed\n");
		exit(1);
	}
	st->roc = roc;
	st->s_l = s_l;
	st->s_l_set = s_l_set;
	st->replay_rtp.lix = lix;
	st->replay_rtp.bitmap = bitmap;
	return st;
}

static void state_out(const char *label, const struct srtp_stream *st)
{
	printf("\"%s\":{\"roc\":%u,\"s_l\":%u,\"s_l_set\":%d,\"lix\":%llu,"
	       "\"bitmap\":%llu}", label, st->roc, st->s_l, st->s_l_set ? 1 : 0,
	       (unsigned long long)st->replay_rtp.lix,
	       (unsigned long long)st->replay_rtp.bitmap);
}

/* packet k of a case: 12-byte header, 16..32 bytes of payload */
static size_t build(uint8_t *p, uint16_t seq, unsigned k, unsigned salt)
{
	const size_t plen = 16 + (5 * k + salt) % 17;
	const uint32_t ts = 160 * k + salt;
	size_t i;
	p[0] = 0x80;
	p[1] = (uint8_t)(96 | ((k & 1) << 7));
	p[2] = seq >> 8;
	p[3] = seq & 0xff;
	p[4] = ts >> 24; p[5] = ts >> 16; p[6] = ts >> 8; p[7] = ts;
	p[8] = SSRC >> 24; p[9] = (SSRC >> 16) & 0xff; p[10] = (SSRC >> 8) & 0xff;
	p[11] = SSRC & 0xff;
	for (i = 0; i < plen; i++)
		p[12 + i] = (uint8_t)(k * 31 + i * 7 + salt);
	return 12 + plen;
}

/* one reference call on a fresh zeroed mbuf holding in[0:len) at pos 0;
 * out receives max(len, end after) bytes.  Returns the end after. */
static size_t run_op(struct srtp *s, int dec, const uint8_t *in, size_t len,
		     uint8_t *out, int first)
{
	struct mbuf *mb = mbuf_alloc(len + 64);
	size_t rec, end;
	int err;
	memset(mb->buf, 0, mb->size);
	memcpy(mb->buf, in, len);
	mb->pos = 0;
	mb->end = len;
	err = dec ? srtp_decrypt(s, mb) : srtp_encrypt(s, mb);
	rec = mb->end > len ? mb->end : len;
	printf("%s\n  {\"in\":", first ? "" : ",");
	hexout(in, len);
	printf(",\"err\":%d,\"pos\":%zu,\"end\":%zu,\"out\":", err, mb->pos,
	       mb->end);
	hexout(mb->buf, rec);
	printf("}");
	memcpy(out, mb->buf, rec);
	end = mb->end;
	mem_deref(mb);
	return end;
}

static int first_case = 1;

static void case_begin(const char *kind, const char *shape, const char *bname,
		       int suite, const uint8_t *key,
		       const struct srtp_stream *st0)
{
	printf("%s\n{\"name\":\"%s_%s_%s_s%d\",\"kind\":\"%s\",\"suite\":%d,"
	       "\"ssrc\":%u,\"key\":", first_case ? "" : ",", kind, shape, bname,
	       suite, kind, suite, SSRC);
	first_case = 0;
	hexout(key, keylen[suite]);
	putchar(',');
	state_out("state0", st0);
	printf(",\"batches\":[");
}

static void alloc_or_die(struct srtp **sp, int suite, const uint8_t *key)
{
	if (srtp_alloc(sp, suite, key, keylen[suite], 0)) {
		fprintf(stderr, "srtp_alloc failed\n");
		exit(1);
	}
}

/* the index the reference's window holds for (roc, seq): misc.c:40 */
static uint64_t ref_lix(uint32_t roc, uint16_t seq)
{
	const int v = (int)roc;
	return seq + v * (uint64_t)65536;
}

static void tx_case(unsigned b, int suite)
{
	uint8_t key[64], pkt[128], out[192];
	struct srtp *tx;
	struct srtp_stream *st;
	unsigned k, batch;
	make_key(key, suite, b);
	alloc_or_die(&tx, suite, key);
	st = stream_at(tx, bounds[b].roc, S_L0, 1, 0, 0);
	case_begin("tx", "in_order", bounds[b].name, suite, key, st);
	for (batch = 0, k = 0; batch < 2; batch++) {
		const unsigned stop = batch ? NPKT : 12;
		int first = 1;
		printf("%s\n {\"ops\":[", batch ? "," : "");
		for (; k < stop; k++) {
			const size_t n = build(pkt, (uint16_t)(S_L0 + 1 + k), k,
					       b + suite);
			run_op(tx, 0, pkt, n, out, first);
			first = 0;
		}
		printf("],");
		state_out("state", st);
		putchar('}');
	}
	printf("]}");
	mem_deref(tx);
}

struct shape {
	const char *name;
	int n[2];               /* arrivals of the two batches */
	int k[2][12];           /* send positions */
};

/* send position 4 is seq 65535, 5 is seq 0 behind the boundary */
static const struct shape shapes[] = {
	{"in_order", {12, 5}, {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
			       {10, 12, 13, 3, 14}}},
	{"swap_across", {9, 5}, {{0, 1, 2, 3, 5, 4, 6, 7, 8},
				 {8, 9, 5, 10, 4}}},
	{"late_before", {9, 5}, {{0, 1, 2, 4, 5, 6, 3, 7, 8},
				 {9, 3, 10, 7, 11}}},
	{"dup_both_sides", {10, 6}, {{0, 1, 1, 2, 3, 4, 5, 6, 6, 7},
				     {4, 8, 5, 9, 9, 10}}},
	{"gap", {7, 6}, {{0, 1, 2, 8, 9, 7, 10}, {3, 11, 5, 8, 12, 13}}},
	{"nine", {9, 6}, {{0, 1, 3, 2, 4, 5, 7, 6, 8}, {6, 9, 10, 1, 11, 10}}},
};

/* roc0 / s_l0: the sender's and the receiver's state before the case */
static void rx_case(const char *bname, const struct shape *sh, int suite,
		    unsigned salt, uint32_t roc0, uint16_t s_l0, uint64_t lix0,
		    uint64_t bitmap0)
{
	uint8_t key[64], pkt[128], prot[NPKT][192], out[192];
	size_t plen[NPKT];
	struct srtp *tx, *rx;
	struct srtp_stream *st;
	int k, batch;
	/* the sender's packets (its calls are not recorded) */
	make_key(key, suite, salt);
	alloc_or_die(&tx, suite, key);
	alloc_or_die(&rx, suite, key);
	stream_at(tx, roc0, s_l0, 1, 0, 0);
	for (k = 0; k < NPKT; k++) {
		struct mbuf *mb = mbuf_alloc(192);
		const size_t n = build(pkt, (uint16_t)(s_l0 + 1 + k), k, salt);
		memset(mb->buf, 0, mb->size);
		memcpy(mb->buf, pkt, n);
		mb->end = n;
		if (srtp_encrypt(tx, mb)) {
			fprintf(stderr, "sender failed\n");
			exit(1);
		}
		plen[k] = mb->end;
		memcpy(prot[k], mb->buf, mb->end);
		mem_deref(mb);
	}
	st = stream_at(rx, roc0, s_l0, 1, lix0, bitmap0);
	case_begin("rx", sh->name, bname, suite, key, st);
	for (batch = 0; batch < 2; batch++) {
		int i;
		printf("%s\n {\"ops\":[", batch ? "," : "");
		for (i = 0; i < sh->n[batch]; i++) {
			k = sh->k[batch][i];
			run_op(rx, 1, prot[k], plen[k], out, i == 0);
		}
		printf("],");
		state_out("state", st);
		putchar('}');
	}
	printf("]}");
	mem_deref(tx);
	mem_deref(rx);
}

int main(void)
{
	static const int rx_suites[2] = {1, 5};
	static const struct shape takeover = {
		"takeover", {6, 5}, {{0, 1, 3, 2, 2, 4}, {3, 5, 6, 0, 7}}};
	unsigned b, s, q;

	printf("{\"generator\":\"oracle/gen_roc_golden.c\",\"cases\":[");
	for (b = 0; b < 3; b++)
		for (s = 0; s < 6; s++)
			tx_case(b, (int)s);
	for (b = 0; b < 3; b++)
		for (s = 0; s < 2; s++)
			for (q = 0; q < sizeof(shapes) / sizeof(shapes[0]); q++)
				rx_case(bounds[b].name, &shapes[q], rx_suites[s],
					16 * b + q, bounds[b].roc, S_L0,
					ref_lix(bounds[b].roc, S_L0), 1);
	/* a stream handed over at a ROC above 2^31 before any packet of it
	 * was received: s_l set, the window still empty */
	for (s = 0; s < 2; s++)
		rx_case("roc80000005", &takeover, rx_suites[s], 99, 0x80000005u,
			1000, 0, 0);
	printf("\n]}\n");
	return 0;
}
