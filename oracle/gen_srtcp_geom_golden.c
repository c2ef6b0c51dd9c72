/*
 * gen_srtcp_geom_golden.c -- reference answers for SRTCP packets of every
 * byte length (TEST INFRASTRUCTURE ONLY).
 *
 * Linked against the reference libre sources compiled by oracle/Makefile
 * (target `ref`).  srtcp_encrypt (srtcp.c:31-140) and srtcp_decrypt
 * (srtcp.c:143-287) take any packet of at least 8 bytes: nothing in them
 * asks for a multiple of 4.  One scenario per suite and per flags in
 * {0, SRTP_UNENCRYPTED_SRTCP}, in the format of gen_golden.c (replayed by
 * tests/golden_util.replay_scenario):
 *
 *   a sender srtcp_encrypts one packet of every length L = LMIN..LMAX in
 *   turn (its SRTCP index runs 1, 2, ...); a receiver with the same flags
 *   srtcp_decrypts each protected packet, in a buffer with no room to spare,
 *   right behind the sender's call; after the last the receiver takes the
 *   packet of length REPEAT again (EALREADY with an HMAC; the reference keeps
 *   no SRTCP replay window without one, srtcp.c:180).
 *
 * A packet's bytes are a fixed function of (L, byte index); no randomness, no
 * time: two runs are identical.
 *
 * Usage: make -C oracle srtcp_geom_golden
 *        (oracle/_ref/gen_srtcp_geom_golden | gzip -9n >
 *         tests/golden/srtcp_geom_golden.json.gz)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <re.h>

#define SSRC   0x67656f6du
#define LMIN   8
#define LMAX   143
#define REPEAT 61
#define ROOM   32               /* the sender's spare room: 4 + 16 at most */

static const size_t keylen[6] = {30, 30, 46, 46, 28, 44};
static const char *opname[2] = {"srtcp_encrypt", "srtcp_decrypt"};

static void hexout(const uint8_t *p, size_t n)
{
	size_t i;
	putchar('"');
	for (i = 0; i < n; i++)
		printf("%02x", p[i]);
	putchar('"');
}

static void make_key(uint8_t *key, int suite, int flags)
{
	size_t i;
	for (i = 0; i < keylen[suite]; i++)
		key[i] = (uint8_t)(37 * i + 11 * suite + 5 * flags + 3);
}

/* the packet of length L: RTCP header (the length field as
 * tests/test_gpu_srtcp.py rtcp_packet writes it; the reference does not read
 * it), the SSRC, the body */
static void build(uint8_t *p, size_t L)
{
	const size_t words = L / 4 - 1;
	size_t i;
	p[0] = 0x81;
	p[1] = (uint8_t)(200 + L % 5);
	p[2] = (uint8_t)(words >> 8);
	p[3] = (uint8_t)words;
	p[4] = SSRC >> 24; p[5] = (SSRC >> 16) & 0xff; p[6] = (SSRC >> 8) & 0xff;
	p[7] = SSRC & 0xff;
	for (i = 8; i < L; i++)
		p[i] = (uint8_t)(L * 29 + i * 7 + (i >> 4) * 3 + 1);
}

static int first_op;

/* one reference call on a fresh mbuf of `size` bytes holding in[0:end) at pos
 * 0, zero behind; out receives max(end, end after) bytes.  Returns the end
 * after. */
static size_t run_op(struct srtp *s, int ctx, int dec, const uint8_t *in,
		     size_t size, size_t end, uint8_t *out, int *errp)
{
	struct mbuf *mb = mbuf_alloc(size);
	size_t rec, e;
	int err;

	memset(mb->buf, 0, mb->size);
	memcpy(mb->buf, in, end);
	mb->pos = 0;
	mb->end = end;
	err = dec ? srtcp_decrypt(s, mb) : srtcp_encrypt(s, mb);
	rec = mb->end > end ? mb->end : end;
	printf("%s\n {\"ctx\":%d,\"op\":\"%s\",\"size\":%zu,\"pos\":0,"
	       "\"end\":%zu,\"in\":", first_op ? "" : ",", ctx, opname[dec],
	       size, end);
	first_op = 0;
	hexout(in, end);
	printf(",\"err\":%d,\"pos_o\":%zu,\"end_o\":%zu,\"size_o\":%zu,"
	       "\"out\":", err, mb->pos, mb->end, mb->size);
	hexout(mb->buf, rec);
	printf("}");
	memcpy(out, mb->buf, rec);
	e = mb->end;
	if (errp)
		*errp = err;
	mem_deref(mb);
	return e;
}

static void scenario(int suite, int flags, int first)
{
	uint8_t key[64], pkt[LMAX], prot[LMAX + ROOM], out[LMAX + ROOM];
	uint8_t again[LMAX + ROOM];
	size_t again_len = 0, L, i;
	struct srtp *tx = NULL, *rx = NULL;
	int err;

	make_key(key, suite, flags);
	if (srtp_alloc(&tx, suite, key, keylen[suite], flags) ||
	    srtp_alloc(&rx, suite, key, keylen[suite], flags)) {
		fprintf(stderr, "srtp_alloc failed\n");
		exit(1);
	}
	printf("%s\n{\"name\":\"srtcp_geom_s%d_f%d\",\"ctxs\":[", first ? "" : ",",
	       suite, flags);
	for (i = 0; i < 2; i++) {
		printf("%s{\"suite\":%d,\"flags\":%d,\"key\":", i ? "," : "",
		       suite, flags);
		hexout(key, keylen[suite]);
		putchar('}');
	}
	printf("],\"ops\":[");
	first_op = 1;
	for (L = LMIN; L <= LMAX; L++) {
		size_t n;
		build(pkt, L);
		n = run_op(tx, 0, 0, pkt, L + ROOM, L, prot, &err);
		if (err) {
			fprintf(stderr, "sender failed at %zu: %d\n", L, err);
			exit(1);
		}
		if (L == REPEAT) {
			memcpy(again, prot, n);
			again_len = n;
		}
		run_op(rx, 1, 1, prot, n, n, out, NULL);
	}
	run_op(rx, 1, 1, again, again_len, again_len, out, NULL);
	printf("]}");
	mem_deref(tx);
	mem_deref(rx);
}

int main(void)
{
	static const int flagv[2] = {0, SRTP_UNENCRYPTED_SRTCP};
	int s, f;

	printf("{\"generator\":\"oracle/gen_srtcp_geom_golden.c\","
	       "\"lengths\":[%d,%d],\"repeat\":%d,\"scenarios\":[", LMIN, LMAX,
	       REPEAT);
	for (s = 0; s < 6; s++)
		for (f = 0; f < 2; f++)
			scenario(s, flagv[f], s == 0 && f == 0);
	printf("\n]}\n");
	return 0;
}
