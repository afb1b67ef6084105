/*
 * TEST INFRASTRUCTURE — fixture generator only (tests/rejection/make_ts_fixture.py
 * runs it once; its output is committed as tests/golden/ts_rejection_f64.json).
 * Never built into or called by the product path.
 *
 * Brute-forces eight bytes of an XofTurboShake128 message (oracle/xof.py:
 * le16(len(dst)) || dst || u8(len(seed)) || seed || binder, domain byte 0x01)
 * so that the Field64 next_vec stream has a candidate >= p = 2^64 - 2^32 + 1
 * among its first <count> candidates, i.e. a little-endian 8-byte word whose
 * top 32 bits are all ones and whose low 32 bits are not zero.  The message
 * must fit one 168-byte absorb block; the Keccak-p[1600, 12] permutation is
 * the oracle's own (oracle/prims.c, included as source).
 *
 *   find_ts_rejection <message hex> <counter offset> <count> <threads>
 * The eight message bytes at <counter offset> are replaced by le64(counter).
 * prints: <counter> <candidate index> <trials>
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/prims.c"

#define RATE 168
#define CHUNK 4096ULL

static uint8_t MSG[RATE];
static int MSG_LEN, CTR_OFF, COUNT, THREADS;
static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static uint64_t next_chunk = 0;
static uint64_t best_ctr = UINT64_MAX;
static int best_cand = -1;

/* candidate index of the first word >= p among the first COUNT, or -1 */
static int scan(uint64_t ctr) {
    uint8_t block[RATE];
    uint64_t st[25];
    memcpy(block, MSG, RATE);
    for (int i = 0; i < 8; i++) block[CTR_OFF + i] = (uint8_t)(ctr >> (8 * i));
    memset(st, 0, sizeof(st));
    for (int i = 0; i < RATE; i++) st[i / 8] ^= (uint64_t)block[i] << (8 * (i % 8));
    oracle_keccak_p1600_12(st);
    for (int j = 0; j < COUNT; j++) {
        const int w = j % (RATE / 8);
        if (j > 0 && w == 0) oracle_keccak_p1600_12(st);
        if ((st[w] >> 32) == 0xffffffffULL && (uint32_t)st[w] != 0) return j;
    }
    return -1;
}

static void* worker(void* arg) {
    (void)arg;
    for (;;) {
        pthread_mutex_lock(&mu);
        const uint64_t c0 = next_chunk;
        const int done = c0 > best_ctr;  /* every counter below the hit has been handed out */
        if (!done) next_chunk += CHUNK;
        pthread_mutex_unlock(&mu);
        if (done) return NULL;
        for (uint64_t ctr = c0; ctr < c0 + CHUNK; ctr++) {
            const int j = scan(ctr);
            if (j < 0) continue;
            pthread_mutex_lock(&mu);
            if (ctr < best_ctr) {
                best_ctr = ctr;
                best_cand = j;
            }
            pthread_mutex_unlock(&mu);
            break;
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: find_ts_rejection message_hex counter_offset count threads\n");
        return 2;
    }
    MSG_LEN = (int)strlen(argv[1]) / 2;
    CTR_OFF = atoi(argv[2]);
    COUNT = atoi(argv[3]);
    THREADS = atoi(argv[4]);
    if (MSG_LEN >= RATE || CTR_OFF < 0 || CTR_OFF + 8 > MSG_LEN || COUNT < 1 || THREADS < 1 || THREADS > 256) {
        fprintf(stderr, "find_ts_rejection: bad arguments\n");
        return 2;
    }
    memset(MSG, 0, RATE);
    for (int i = 0; i < MSG_LEN; i++) {
        unsigned v;
        sscanf(argv[1] + 2 * i, "%2x", &v);
        MSG[i] = (uint8_t)v;
    }
    MSG[MSG_LEN] ^= 0x01;   /* TurboSHAKE domain byte */
    MSG[RATE - 1] ^= 0x80;  /* pad10*1 */
    pthread_t th[256];
    for (int t = 0; t < THREADS; t++) pthread_create(&th[t], NULL, worker, NULL);
    for (int t = 0; t < THREADS; t++) pthread_join(th[t], NULL);
    /* the smallest counter with a hit: every chunk below it was scanned to the end */
    printf("%llu %d %llu\n", (unsigned long long)best_ctr, best_cand, (unsigned long long)next_chunk);
    return 0;
}
