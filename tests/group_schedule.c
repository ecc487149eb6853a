/*
 * group_schedule.c -- the union-find of nbody_amd/csrc/group_common.h held to its argument over schedules, without a GPU.
 *
 * The program compiles nb_group_find and nb_group_unite as they stand in the header (NB_GROUP_OPS_HEADER puts its own three
 * operations under them, group_schedule_ops.h) and runs them on logical threads: coroutines (ucontext), never OS threads.  Every
 * NB_GROUP_LOAD, NB_GROUP_CAS and NB_GROUP_MIN first yields to a scheduler, which picks the thread whose pending operation acts
 * next.  With stale loads (argument 4 in its strongest reading) a load of parent[x] returns ANY value the word has ever held,
 * picked by the scheduler too; compare-and-swap and minimum act on the current memory.
 *
 * Thread bodies, one per caller of the statement:
 *   host    group_cpu.c's: per receiver a kept root; rj = find(j); if (rj != root) root = unite(root, rj)
 *   device  fetch() of group.hip, restated (it sits beside __ballot and cannot be compiled here): two receivers per thread, as a
 *           lane holds; the fetch's parent[j] loaded first, all of them; a source is skipped where every linked receiver's kept
 *           root equals pj; else rj = find(pj) and each linked receiver whose root differs unites and keeps what returns
 *
 * Checked after every operation: a stored value never exceeds the word's previous value, never its own index, and is a node of
 * the same component of the link graph.  Per call: find ends within x hops (at most 3 operations a hop), unite within the rounds
 * argument 3 allows, and what unite returns is of the joined component and not above either argument.  At the end: a sequential
 * flatten gives every node the smallest index of its component, computed here by a plain sequential union-find.  A run that
 * exceeds its operation budget fails as "does not terminate".
 *
 * Modes: `exhaustive` walks every scheduler choice depth-first by replay, on the tiny cases below; `random` draws the choices
 * from a seeded generator on 32 to 64 nodes and 8 threads.  GROUP_VARIANT_HEADER, when defined, names a file with copies of the
 * two functions called variant_find and variant_unite (tests/test_group_schedule.py plants one defect in each copy): the same
 * program must then report a failure.
 *
 *   group_schedule host|device stale|fresh exhaustive CASE
 *   group_schedule host|device stale|fresh random chain|clique|two_chains NODES THREADS SEED RUNS
 * Prints one line, "OK ..." (exit 0), "FAIL ..." (exit 1) or "CUT ..." (exit 2: an exhaustive walk that was not finished).
 */
#define _XOPEN_SOURCE 700
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#define NB_GROUP_OPS_HEADER "group_schedule_ops.h"
#include "group_common.h"

#ifdef GROUP_VARIANT_HEADER
#include GROUP_VARIANT_HEADER
#define FIND variant_find
#define UNITE variant_unite
#else
#define FIND nb_group_find
#define UNITE nb_group_unite
#endif

enum { MAXN = 64, MAXT = 8, MAXL = 2048, MAXD = 1 << 16, FETCH = 8, STACK = 64 * 1024 };

typedef struct {
    uint32_t i, j;
} Link;

/* the case */
static uint32_t g_n;
static int g_threads;
static Link g_links[MAXT][MAXL];
static int g_nlinks[MAXT];
static uint32_t g_comp[MAXN]; /* smallest index of the component of the link graph */
static int g_device, g_stale, g_random;
static char g_label[128];

/* the run */
static uint32_t parent[MAXN];
static uint32_t g_hist[MAXN][MAXN + 1]; /* every value the word has held, oldest first */
static int g_nhist[MAXN];
static uint64_t g_ops, g_budget, g_thread_ops[MAXT];
static uint64_t g_schedules, g_most_ops, g_stale_roots; /* g_stale_roots: returns of unite that were no root any more */

/* the scheduler */
static ucontext_t g_main, g_ctx[MAXT];
static char *g_stack[MAXT];
static int g_alive[MAXT], g_started[MAXT], g_nalive, g_cur, g_grant;
static int g_path[MAXD], g_width[MAXD], g_depth, g_replay;
static uint64_t g_rng;

static void fail(const char *what, uint32_t a, uint32_t b, uint32_t c) {
    printf("FAIL %s: %s (%u, %u, %u) in schedule %llu after %llu operations; choices", g_label, what, a, b, c,
           (unsigned long long)g_schedules, (unsigned long long)g_ops);
    if (!g_random)
        for (int d = 0; d < g_depth && d < 64; d++) printf(" %d/%d", g_path[d], g_width[d]);
    printf("\n");
    exit(1);
}

static uint64_t rng_next(uint64_t *s) { /* splitmix64 */
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* one of n options: the next of the replayed path, a first visit (0), or a draw */
static int choose(int n) {
    if (n <= 1) return 0;
    if (g_random) return (int)(rng_next(&g_rng) % (uint64_t)n);
    if (g_depth >= MAXD) fail("does not terminate (choice depth)", (uint32_t)g_depth, 0, 0);
    const int c = g_depth < g_replay ? g_path[g_depth] : 0;
    g_path[g_depth] = c;
    g_width[g_depth] = n;
    g_depth++;
    return c;
}

/* hands the processor to the thread whose pending operation acts next; returns in the caller once it is chosen again */
static void pick(int me) {
    int ids[MAXT], k = 0;
    for (int t = 0; t < g_threads; t++)
        if (g_alive[t]) ids[k++] = t;
    const int next = ids[choose(k)];
    if (next == me) return;
    if (!g_started[next]) { /* it runs from its start to its first operation, which is the one that was chosen */
        g_started[next] = 1;
        g_grant = 1;
    }
    g_cur = next;
    swapcontext(me < 0 ? &g_main : &g_ctx[me], &g_ctx[next]);
}

static void yield_point(void) {
    if (++g_ops > g_budget) fail("does not terminate (operation budget)", (uint32_t)g_budget, 0, 0);
    g_thread_ops[g_cur]++;
    if (g_grant) {
        g_grant = 0;
        return;
    }
    pick(g_cur);
}

static uint32_t word(const uint32_t *p) {
    const size_t x = (size_t)(p - parent);
    if (p < parent || x >= g_n) fail("an access outside the table", (uint32_t)x, 0, 0);
    return (uint32_t)x;
}

static void store(uint32_t x, uint32_t v) {
    if (v >= g_n) fail("a stored value is no index", x, v, 0);
    if (v > parent[x]) fail("a stored value exceeds the word's previous value", x, v, parent[x]);
    if (v > x) fail("a stored value is above its own index", x, v, 0);
    if (g_comp[v] != g_comp[x]) fail("a stored value is of another component", x, v, 0);
    parent[x] = v;
    for (int h = 0; h < g_nhist[x]; h++)
        if (g_hist[x][h] == v) return;
    g_hist[x][g_nhist[x]++] = v;
}

uint32_t gs_load(const uint32_t *p) {
    yield_point();
    const uint32_t x = word(p);
    return g_stale ? g_hist[x][choose(g_nhist[x])] : parent[x];
}

uint32_t gs_cas(uint32_t *p, uint32_t expected, uint32_t desired) {
    yield_point();
    const uint32_t x = word(p), old = parent[x];
    if (old == expected) store(x, desired);
    return old;
}

void gs_min(uint32_t *p, uint32_t v) {
    yield_point();
    const uint32_t x = word(p);
    if (v < parent[x]) store(x, v);
}

void gs_store(uint32_t *p, uint32_t v) {
    yield_point();
    store(word(p), v);
}

/* find(x): every hop but the last lowers x, and a hop is at most two loads and a minimum (argument 2) */
static uint32_t checked_find(uint32_t x) {
    const uint64_t before = g_thread_ops[g_cur];
    const uint32_t r = FIND(parent, x);
    const uint64_t used = g_thread_ops[g_cur] - before;
    if (used > 3ull * x + 1) fail("find took more than x hops", x, (uint32_t)used, 0);
    if (r > x || g_comp[r] != g_comp[x]) fail("find returned a node above x or of another component", x, r, 0);
    return r;
}

/* unite(a, b): max(a, b) strictly falls at every failed round (argument 3), a round is two finds and a compare-and-swap */
static uint32_t checked_unite(uint32_t a, uint32_t b) {
    const uint64_t before = g_thread_ops[g_cur];
    const uint32_t r = UNITE(parent, a, b);
    const uint64_t used = g_thread_ops[g_cur] - before;
    const uint64_t rounds = (uint64_t)(a > b ? a : b) + 1;
    if (used > rounds * (3ull * a + 3ull * b + 3)) fail("unite took more rounds than max(a, b) allows", a, b, (uint32_t)used);
    if (r > a || r > b) fail("unite returned a node above an argument", a, b, r);
    if (g_comp[r] != g_comp[a] || g_comp[r] != g_comp[b]) fail("unite returned a node of another component", a, b, r);
    g_stale_roots += parent[r] != r; /* counted, not a failure: no caller needs a root, only a node of the tree not above a or b */
    return r;
}

/* group_cpu.c's loop body: the receivers of this thread one after another, the linked sources of each in the list's order */
static void host_body(int t) {
    uint32_t root = 0, receiver = UINT32_MAX;
    for (int l = 0; l < g_nlinks[t]; l++) {
        const uint32_t i = g_links[t][l].i, j = g_links[t][l].j;
        if (i != receiver) receiver = root = i;
        const uint32_t rj = checked_find(j);
        if (rj != root) root = checked_unite(root, rj);
    }
}

/*
 * fetch() of nbody_amd/csrc/group.hip, from "uint32_t pj[S]" to its end, restated: the thread is a lane with K = 2 receivers;
 * its links are taken two receivers at a time (in the order the list first names them), the sources those two link to in the
 * order the list first names them, FETCH = 8 to a fetch; hits is the kernel's bit u * K + k.
 */
static void device_body(int t) {
    const int n = g_nlinks[t];
    static char taken[MAXT][MAXL];
    char *done = taken[t];
    memset(done, 0, (size_t)n);
    for (int first = 0; first < n; first++) {
        if (done[first]) continue;
        uint32_t ri[2] = {g_links[t][first].i, g_links[t][first].i};
        int have = 1;
        for (int l = first; l < n && have < 2; l++)
            if (!done[l] && g_links[t][l].i != ri[0]) ri[have++] = g_links[t][l].i;
        uint32_t src[MAXN], hit[MAXN];
        int ns = 0;
        for (int l = first; l < n; l++) {
            if (done[l]) continue;
            const uint32_t i = g_links[t][l].i, j = g_links[t][l].j;
            const int k = i == ri[0] ? 0 : (have == 2 && i == ri[1]) ? 1 : -1;
            if (k < 0) continue;
            done[l] = 1;
            int u = 0;
            while (u < ns && src[u] != j) u++;
            if (u == ns) src[ns] = j, hit[ns] = 0, ns++;
            hit[u] |= 1u << k;
        }
        uint32_t root[2] = {ri[0], ri[1]}; /* a particle is of its own tree */
        for (int f = 0; f < ns; f += FETCH) {
            const int s = ns - f < FETCH ? ns - f : FETCH;
            uint32_t pj[FETCH];
            for (int u = 0; u < s; u++) pj[u] = NB_GROUP_LOAD(parent + src[f + u]);
            for (int u = 0; u < s; u++) {
                int apart = 0;
                for (int k = 0; k < 2; k++) apart = apart || (((hit[f + u] >> k) & 1u) && root[k] != pj[u]);
                if (!apart) continue;
                const uint32_t rj = checked_find(pj[u]);
                for (int k = 0; k < 2; k++)
                    if (((hit[f + u] >> k) & 1u) && root[k] != rj) root[k] = checked_unite(root[k], rj);
            }
        }
    }
}

static void thread_main(int t) {
    if (g_device)
        device_body(t);
    else
        host_body(t);
    g_alive[t] = 0;
    if (--g_nalive == 0) {
        g_cur = -1;
        setcontext(&g_main);
    }
    pick(t); /* never chosen again */
    abort();
}

static void run_once(void) {
    for (uint32_t x = 0; x < g_n; x++) parent[x] = x, g_hist[x][0] = x, g_nhist[x] = 1;
    g_ops = 0;
    g_depth = 0;
    g_grant = 0;
    g_nalive = 0;
    for (int t = 0; t < g_threads; t++) {
        g_thread_ops[t] = 0;
        g_started[t] = 0;
        g_alive[t] = g_nlinks[t] > 0;
        g_nalive += g_alive[t];
        g_ctx[t].uc_stack.ss_sp = g_stack[t];
        g_ctx[t].uc_stack.ss_size = STACK;
        g_ctx[t].uc_link = &g_main;
        makecontext(&g_ctx[t], (void (*)(void))thread_main, 1, t);
    }
    if (g_nalive) pick(-1);
    /* every thread has ended: the sequential flatten */
    for (uint32_t x = 0; x < g_n; x++) {
        uint32_t r = x, hops = 0;
        while (parent[r] != r) {
            if (parent[r] > r || ++hops > g_n) fail("the final table has a cycle or a rising entry", x, r, parent[r]);
            r = parent[r];
        }
        if (r != g_comp[x]) fail("a node does not end at the smallest index of its component", x, r, g_comp[x]);
    }
    g_schedules++;
    if (g_ops > g_most_ops) g_most_ops = g_ops;
}

/* ---- the cases ---------------------------------------------------------------------------------------------------------------- */

static void add(int t, uint32_t a, uint32_t b) {
    if (a == b) return;
    if (g_nlinks[t] >= MAXL) fail("too many links for a thread", (uint32_t)t, 0, 0);
    g_links[t][g_nlinks[t]].i = a > b ? a : b; /* the receiver is the larger index, as in both callers */
    g_links[t][g_nlinks[t]].j = a > b ? b : a;
    g_nlinks[t]++;
}

typedef struct {
    const char *name;
    uint32_t n;
    int threads;
    int links[8][3]; /* thread, a, b; ends at thread -1 */
} Tiny;

static const Tiny TINY[] = {
    {"two_hooks_3", 3, 2, {{0, 1, 2}, {1, 0, 2}, {-1}}},
    {"triangle_3", 3, 3, {{0, 0, 1}, {1, 1, 2}, {2, 0, 2}, {-1}}},
    {"shared_source_3", 3, 2, {{0, 2, 0}, {0, 1, 0}, {1, 2, 1}, {-1}}}, /* the device shape: one lane's two receivers link to one source */
    {"crossed_pairs_4", 4, 2, {{0, 3, 2}, {0, 1, 0}, {1, 2, 1}, {1, 3, 0}, {-1}}},
    {"chain_4", 4, 3, {{0, 3, 2}, {1, 2, 1}, {2, 1, 0}, {-1}}},
    {"star_4", 4, 3, {{0, 3, 0}, {1, 3, 1}, {2, 3, 2}, {-1}}},
    {"two_components_4", 4, 3, {{0, 3, 1}, {1, 2, 0}, {2, 3, 1}, {-1}}}, /* {0, 2} and {1, 3}: two threads on one link */
};

static int tiny_case(const char *name) {
    for (size_t c = 0; c < sizeof TINY / sizeof TINY[0]; c++) {
        if (strcmp(TINY[c].name, name) != 0) continue;
        g_n = TINY[c].n;
        g_threads = TINY[c].threads;
        for (int l = 0; l < 8 && TINY[c].links[l][0] >= 0; l++) add(TINY[c].links[l][0], (uint32_t)TINY[c].links[l][1], (uint32_t)TINY[c].links[l][2]);
        return 1;
    }
    return 0;
}

/* the links of a seeded world: host receivers are dealt whole to a thread (group_cpu.c), device links one by one (a receiver's
 * sources are split over the waves and spans of the launch, each with a kept root of its own) */
static void random_case(const char *kind, uint32_t n, int threads, uint64_t seed) {
    static Link all[MAXL];
    int count = 0;
    uint64_t s = seed * 0x2545f4914f6cdd1dull + 1;
    uint32_t perm[MAXN];
    for (uint32_t x = 0; x < n; x++) perm[x] = x;
    for (uint32_t x = n - 1; x > 0; x--) {
        const uint32_t y = (uint32_t)(rng_next(&s) % (x + 1)), v = perm[x];
        perm[x] = perm[y], perm[y] = v;
    }
#define LINK(a, b) (all[count].i = (a) > (b) ? (a) : (b), all[count].j = (a) > (b) ? (b) : (a), count++)
    if (strcmp(kind, "chain") == 0) {
        for (uint32_t x = 0; x + 1 < n; x++) LINK(perm[x], perm[x + 1]);
        for (uint32_t x = 0; x < n / 2; x++) {
            const uint32_t a = (uint32_t)(rng_next(&s) % n), b = (uint32_t)(rng_next(&s) % n);
            if (a != b) LINK(a, b);
        }
    } else if (strcmp(kind, "clique") == 0) {
        for (uint32_t a = 1; a < n; a++)
            for (uint32_t b = 0; b < a; b++) LINK(a, b);
    } else if (strcmp(kind, "two_chains") == 0) {
        for (uint32_t x = 0; x + 2 < n; x++) LINK(perm[x], perm[x + 2]);
    } else {
        fail("unknown kind of world", 0, 0, 0);
    }
#undef LINK
    g_n = n;
    g_threads = threads;
    if (g_device) {
        for (int l = count - 1; l > 0; l--) { /* shuffled, then dealt round robin */
            const int y = (int)(rng_next(&s) % (uint64_t)(l + 1));
            const Link v = all[l];
            all[l] = all[y], all[y] = v;
        }
        for (int l = 0; l < count; l++) add(l % threads, all[l].i, all[l].j);
    } else {
        int owner[MAXN];
        for (uint32_t x = 0; x < n; x++) owner[x] = (int)(rng_next(&s) % (uint64_t)threads);
        for (uint32_t i = 0; i < n; i++) /* per receiver the sources in ascending order, as the scan meets them */
            for (uint32_t j = 0; j < i; j++)
                for (int l = 0; l < count; l++)
                    if (all[l].i == i && all[l].j == j) {
                        add(owner[i], i, j);
                        break;
                    }
    }
}

static void components(void) {
    uint32_t up[MAXN];
    for (uint32_t x = 0; x < g_n; x++) up[x] = x;
    for (int t = 0; t < g_threads; t++)
        for (int l = 0; l < g_nlinks[t]; l++) {
            uint32_t a = g_links[t][l].i, b = g_links[t][l].j;
            while (up[a] != a) a = up[a];
            while (up[b] != b) b = up[b];
            if (a != b) up[a > b ? a : b] = a > b ? b : a;
        }
    for (uint32_t x = 0; x < g_n; x++) {
        uint32_t r = x;
        while (up[r] != r) r = up[r];
        g_comp[x] = r;
    }
}

int main(int argc, char **argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s host|device stale|fresh exhaustive CASE | random KIND NODES THREADS SEED RUNS\n", argv[0]);
        return 64;
    }
    g_device = strcmp(argv[1], "device") == 0;
    g_stale = strcmp(argv[2], "stale") == 0;
    g_random = strcmp(argv[3], "random") == 0;
    uint64_t seed = 0, runs = 0, cut = 200000000ull;
    if (g_random) {
        if (argc < 9) return 64;
        const uint32_t n = (uint32_t)atoi(argv[5]);
        const int threads = atoi(argv[6]);
        if (n < 2 || n > MAXN || threads < 1 || threads > MAXT) return 64;
        seed = strtoull(argv[7], NULL, 10);
        runs = strtoull(argv[8], NULL, 10);
        snprintf(g_label, sizeof g_label, "%s %s random %s n=%u threads=%d seed=%llu", argv[1], argv[2], argv[4], n, threads, (unsigned long long)seed);
        random_case(argv[4], n, threads, seed);
    } else {
        if (argc > 5) cut = strtoull(argv[5], NULL, 10);
        snprintf(g_label, sizeof g_label, "%s %s exhaustive %s", argv[1], argv[2], argv[4]);
        if (!tiny_case(argv[4])) {
            fprintf(stderr, "unknown case %s\n", argv[4]);
            return 64;
        }
    }
    components();
    uint64_t links = 0;
    for (int t = 0; t < g_threads; t++) links += (uint64_t)g_nlinks[t];
    /* generous: a link costs a find and a unite of a few rounds when nothing goes wrong, a few dozen operations */
    g_budget = 1000 + 400 * links * (g_random ? g_n : 1);
    for (int t = 0; t < g_threads; t++) {
        g_stack[t] = malloc(STACK);
        if (!g_stack[t] || getcontext(&g_ctx[t]) != 0) return 70;
    }
    int ended = 0;
    if (g_random) {
        for (uint64_t r = 0; r < runs; r++) {
            g_rng = seed * 1000003ull + r;
            run_once();
        }
        ended = 1;
    } else {
        g_replay = 0;
        while (g_schedules < cut) {
            run_once();
            while (g_depth > 0 && g_path[g_depth - 1] + 1 >= g_width[g_depth - 1]) g_depth--;
            if (g_depth == 0) {
                ended = 1;
                break;
            }
            g_path[g_depth - 1]++;
            g_replay = g_depth;
        }
    }
    printf("%s %s: %llu schedules%s, at most %llu operations in one, %llu links, %llu returns of unite no longer a root\n",
           ended ? "OK" : "CUT", g_label, (unsigned long long)g_schedules, g_random ? "" : ended ? ", exhausted" : ", not exhausted",
           (unsigned long long)g_most_ops, (unsigned long long)links, (unsigned long long)g_stale_roots);
    for (int t = 0; t < g_threads; t++) free(g_stack[t]);
    return ended ? 0 : 2;
}
