// aptai_ctc_beam_search: flashlight's lexicon-free CTC beam search without a language model, on the device (contract and tie
// rule: include/aptai_hip.h; aptai_amd/hostlogic.py ctc_beam_search is the same search in Python and the tests' oracle).
//
// One workgroup of four waves per utterance, frames in sequence.  Per frame:
//   1  every thread: token beam (rank of each logit), the slots that share a history (twin), the slots holding the parent history
//      of a slot (pa / pb) and, per token, the slots whose history ends in it (mprev): all the merge partners a candidate can have.
//   2  every wave: its share of the nh x na candidates.  A candidate's score is (hs + x) + bonus in fp64; it looks up its at most two
//      partners (see eval_cand), and only the best of a state stays alive, carrying the merged score.  A wave keeps its 32 best in
//      registers: a batch of 64 candidates is sorted over the lanes (bitonic network on shuffles), its best 32 join the upper lanes
//      worst first, and six merge stages put the best 32 of both below.
//   3  wave 0: merges the four waves' lists the same way, resolves the history node of each survivor (hash lookup, allocation by
//      lane rank: no atomics), writes the next beam and the frame's back-pointers.
// Histories are nodes (parent, token) of a trie in the workspace, found through a chained hash table keyed by (parent, token): equal
// token sequences have equal node ids for the whole utterance, also when a history left the beam and is reached again.
// aptai_ctc_beam_search_lm is the second instantiation of the same kernel (template <bool LM>): a token n-gram compiled to a dense
// automaton (aptai_amd/ngram.py) adds lm_w[state][n] to every candidate that extends its history.  The state of a history lives in
// the fourth int of its trie node and, per beam slot, in LDS; the frame maximum, which slot 0 no longer has to reach, is a pass over
// all candidates in front of step 2.  The nh table rows of a frame are read straight through L2 (DESIGN.md has the reasoning).
// Memory: trie, hash heads, back-pointers and token rows are written and read by this workgroup only, always with a __syncthreads()
// between (workgroup scope is enough).
#include <math.h>

#include "common.h"

namespace {

constexpr int MAXV = APTAI_BEAM_MAX_V;
constexpr int BMAX = APTAI_BEAM_MAX;
constexpr int NTHREADS = 256;
constexpr int NWAVES = NTHREADS / 64;
constexpr uint32_t DEAD = 0xffffffffu;
static_assert(BMAX == 32, "a wave's lower half holds one beam; mprev is a 32-bit slot mask");

struct BeamArgs {
    const float* logits;
    long ldl, rows_per_b;
    const int32_t* input_lens;
    int T, V, blank, sil, beam, ktok, log_add, nbest, max_n;
    double thr, sil_score;
    int4* nodes;        // per utterance node_cap entries {parent node, token, next in hash chain, LM state (0 without an LM)}
    int* heads;         // per utterance n_heads (power of two) chain heads, -1 = empty
    uint16_t* bp;       // per utterance [T][beam]  (parent slot << 8) | token
    uint8_t* rows;      // per utterance [nbest][T + 2] token rows of the hypotheses read out
    long node_cap, n_heads;
    int32_t *tokens, *timesteps, *n_tok, *n_hyp;
    double* score;
};

// the n-gram automaton of aptai_ctc_beam_search_lm, pre-multiplied by the LM weight on the host: w [C][V], next [C][V], wfinal [C]
struct LmArgs {
    const double* w;
    const int32_t* next;
    const double* wfinal;
    int start;
};

struct Key {
    double s;
    uint32_t c;   // (slot << 8) | token, DEAD = no candidate
};

// a before b: higher score, then lower slot, then lower token (the header's tie rule); a dead key (-inf, DEAD) is last
__device__ __forceinline__ bool before(double as, uint32_t ac, double bs, uint32_t bc) { return as > bs || (as == bs && ac < bc); }

// bitonic sort of one key per lane over the wave: lane 0 ends with the first key in `before` order
__device__ __forceinline__ void sort64(double& s, uint32_t& c, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const double os = __shfl_xor(s, j, 64);
            const uint32_t oc = __shfl_xor(c, j, 64);
            const bool want_first = ((lane & j) == 0) == ((lane & k) == 0);
            if (before(os, oc, s, c) == want_first) { s = os; c = oc; }
        }
    }
}

// lanes 32..63 take 32 new keys sorted WORST first (ns, nc valid there) beside the 32 sorted best first in lanes 0..31: the wave holds
// a bitonic row, six merge stages sort it, the best 32 of old and new end in lanes 0..31
__device__ __forceinline__ void merge32(double& rs, uint32_t& rc, double ns, uint32_t nc, int lane) {
    if (lane >= 32) { rs = ns; rc = nc; }
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const double os = __shfl_xor(rs, j, 64);
        const uint32_t oc = __shfl_xor(rc, j, 64);
        if (before(os, oc, rs, rc) == ((lane & j) == 0)) { rs = os; rc = oc; }
    }
}

// numpy's logaddexp for x >= y
__device__ __forceinline__ double logaddexp_ge(double x, double y) { return x == y ? x + M_LN2 : x + log1p(exp(y - x)); }

struct Shared {
    float x[2][MAXV];
    double hs[2][BMAX];                                   // the beam, best first: score, history node, that node's parent,
    int hist[2][BMAX], par[2][BMAX], prev[2][BMAX], flag[2][BMAX];   // last token, last-was-blank
    int twin[BMAX], pa[BMAX], pb[BMAX];
    uint32_t mprev[MAXV];
    int act[MAXV];
    double top_s[NWAVES][32];
    uint32_t top_c[NWAVES][32];
    int nh, pool_n, n_hyp;
};

// with a language model: its state per beam slot, and the waves' shares of the frame maximum
struct SharedLM : Shared {
    int lms[2][BMAX];
    double wmax[NWAVES];
};
template <bool LM> struct SharedOf { typedef Shared type; };
template <> struct SharedOf<true> { typedef SharedLM type; };

// the LM term of token n from slot h, which must extend there: the table arrives multiplied by the LM weight, read through L2
__device__ __forceinline__ double lm_term(const SharedLM& sh, int cur, int h, int n, int V, const LmArgs& lm) {
    return lm.w[sh.lms[cur][h] * V + n];
}

// Score of candidate (slot h, token n) on its own: (hs + x) + bonus in fp64, then, with an LM and where n extends the history
// of h, + lm_w[state][n] as a plain add (no multiply on the device, so nothing for the compiler to fuse).
template <bool LM, typename S>
__device__ __forceinline__ double cand_score(const S& sh, int cur, int h, int n, const BeamArgs& a, const LmArgs& lm) {
    double sc = (sh.hs[cur][h] + (double)sh.x[cur][n]) + (n == a.sil ? a.sil_score : 0.0);
    if constexpr (LM) {
        if (n != a.blank && (n != sh.prev[cur][h] || sh.flag[cur][h])) sc = sc + lm_term(sh, cur, h, n, a.V, lm);
    }
    return sc;
}

// Candidate (slot h, token n) of the frame.  States that can coincide (at most three candidates per state):
//   blank        (hist_h, blank, 1)   <- the blank of the other slot with history hist_h
//   repeat       (hist_h, n, 0)       <- token n from the slots whose history is the parent of hist_h, where it extends
//   extension    (hist_h + n, n, 0)   <- token n from the other slot with history hist_h, where it extends, and the repeat of the
//                                        slot whose history is hist_h + n
// The best of a state (tie: lower slot; the token is the same) returns the merged score, the others return a dead key.
// LM: every partner takes its own term by the rule of cand_score: the twin that extends shares the history, hence the state and
// the term; pa / pb extend from the parent's state; blanks and repeats take none.
template <bool LM, typename S>
__device__ __forceinline__ Key eval_cand(const S& sh, int cur, int h, int n, double floor_, const BeamArgs& a, const LmArgs& lm) {
    const Key dead = {-INFINITY, DEAD};
    const double xs = (double)sh.x[cur][n];
    const double bonus = n == a.sil ? a.sil_score : 0.0;
    const int prev = sh.prev[cur][h], flag = sh.flag[cur][h];
    double sc = (sh.hs[cur][h] + xs) + bonus;
    double t1 = 0.0, t2 = 0.0;       // LM terms of the partners q1, q2
    bool lm1 = false, lm2 = false;
    if constexpr (LM) {
        if (n != a.blank && (n != prev || flag)) {
            t1 = lm_term(sh, cur, h, n, a.V, lm);
            sc = sc + t1;
            lm1 = true;
        }
    }
    if (!(sc >= floor_)) return dead;
    int q1 = -1, q2 = -1;
    if (n == a.blank) {
        q1 = sh.twin[h];
    } else if (n == prev && !flag) {
        int p = sh.pa[h];
        if (p >= 0 && (sh.prev[cur][p] != n || sh.flag[cur][p])) q1 = p;
        p = sh.pb[h];
        if (p >= 0 && (sh.prev[cur][p] != n || sh.flag[cur][p])) q2 = p;
        if constexpr (LM) {
            if (q1 >= 0) { t1 = lm_term(sh, cur, q1, n, a.V, lm); lm1 = true; }
            if (q2 >= 0) { t2 = lm_term(sh, cur, q2, n, a.V, lm); lm2 = true; }
        }
    } else {
        const int p = sh.twin[h];
        if (p >= 0 && (sh.prev[cur][p] != n || sh.flag[cur][p])) q1 = p;
        const int hh = sh.hist[cur][h];
        for (uint32_t m = sh.mprev[n]; m; m &= m - 1) {
            const int c = __ffs(m) - 1;
            if (sh.par[cur][c] == hh) { q2 = c; break; }
        }
    }
    double s1 = -INFINITY, s2 = -INFINITY;
    bool v1 = false, v2 = false;
    if (q1 >= 0) {
        s1 = (sh.hs[cur][q1] + xs) + bonus;
        if constexpr (LM) { if (lm1) s1 = s1 + t1; }
        v1 = s1 >= floor_;
    }
    if (q2 >= 0) {
        s2 = (sh.hs[cur][q2] + xs) + bonus;
        if constexpr (LM) { if (lm2) s2 = s2 + t2; }
        v2 = s2 >= floor_;
    }
    if (v1 && (s1 > sc || (s1 == sc && q1 < h))) return dead;
    if (v2 && (s2 > sc || (s2 == sc && q2 < h))) return dead;
    double m = sc;
    if (a.log_add) {
        if (v1 && v2) {
            m = logaddexp_ge(m, fmax(s1, s2));
            m = logaddexp_ge(m, fmin(s1, s2));
        } else if (v1) {
            m = logaddexp_ge(m, s1);
        } else if (v2) {
            m = logaddexp_ge(m, s2);
        }
    }
    return Key{m, ((uint32_t)h << 8) | (uint32_t)n};
}

__device__ __forceinline__ uint32_t node_hash(int parent, int tok) {
    uint32_t h = (uint32_t)parent * 0x9E3779B1u + (uint32_t)tok * 0x85EBCA6Bu;
    return h ^ (h >> 15);
}

// LM = false is the search without a language model (`lm` is not read); LM = true adds the n-gram automaton `lm`
template <bool LM>
__global__ __launch_bounds__(NTHREADS) void ctc_beam_kernel(BeamArgs a, LmArgs lm) {
    __shared__ typename SharedOf<LM>::type sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, beam = a.beam;
    int Tb = a.input_lens ? a.input_lens[b] : a.T;
    Tb = Tb < 0 ? 0 : (Tb > a.T ? a.T : Tb);
    const float* x0 = a.logits + (long)b * a.rows_per_b * a.ldl;
    int4* nodes = a.nodes + (long)b * a.node_cap;
    int* heads = a.heads + (long)b * a.n_heads;
    uint16_t* bp = a.bp + (long)b * a.T * beam;
    uint8_t* rows = a.rows + (long)b * a.nbest * (a.T + 2);
    const uint32_t hmask = (uint32_t)(a.n_heads - 1);

    for (long i = tid; i < a.n_heads; i += NTHREADS) heads[i] = -1;
    if (tid == 0) {
        nodes[0] = make_int4(-1, a.sil, -1, LM ? lm.start : 0);
        if constexpr (LM) sh.lms[0][0] = lm.start;
        sh.hs[0][0] = 0.0;
        sh.hist[0][0] = 0;
        sh.par[0][0] = -1;
        sh.prev[0][0] = a.sil;
        sh.flag[0][0] = 0;
        sh.nh = 1;
        sh.pool_n = 1;
    }
    if (tid < V) {
        sh.act[tid] = tid;
        if (Tb > 0) sh.x[0][tid] = x0[tid];
    }
    const int na = a.ktok;
    __syncthreads();

    for (int t = 0; t < Tb; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        const int nh = sh.nh;
        float x_next = 0.f;
        if (tid < V && t + 1 < Tb) x_next = x0[(long)(t + 1) * a.ldl + tid];
        // ---- 1: token beam and merge partners
        if (tid < V) {
            if (na < V) {     // rank in the stable descending order: ties to the lower id
                const float xv = sh.x[cur][tid];
                int r = 0;
                for (int m = 0; m < V; ++m) {
                    const float xm = sh.x[cur][m];
                    r += (xm > xv || (xm == xv && m < tid)) ? 1 : 0;
                }
                if (r < na) sh.act[r] = tid;
            }
            uint32_t mk = 0;
            for (int h = 0; h < nh; ++h)
                if (!sh.flag[cur][h] && sh.prev[cur][h] == tid && sh.par[cur][h] >= 0) mk |= 1u << h;
            sh.mprev[tid] = mk;
        }
        if (tid < nh) {
            const int hh = sh.hist[cur][tid];
            const int pp = (!sh.flag[cur][tid]) ? sh.par[cur][tid] : -1;
            int tw = -1, p0 = -1, p1 = -1;
            for (int h = 0; h < nh; ++h) {
                const int o = sh.hist[cur][h];
                if (h != tid && o == hh) tw = h;
                if (pp >= 0 && o == pp) { if (p0 < 0) p0 = h; else p1 = h; }
            }
            sh.twin[tid] = tw;
            sh.pa[tid] = p0;
            sh.pb[tid] = p1;
        }
        __syncthreads();
        // ---- 2: candidates, 32 best per wave.  The frame maximum is reached from slot 0 (the beam is sorted and rounding is monotone)
        // without an LM; with one any slot can reach it: a pass over all nh x na candidates, the waves' maxima meet in LDS.
        const int NC = nh * na;
        double best = -INFINITY;
        if constexpr (LM) {
            for (int idx = tid; idx < NC; idx += NTHREADS) {
                const int h = idx / na;
                best = fmax(best, cand_score<true>(sh, cur, h, sh.act[idx - h * na], a, lm));
            }
        } else {
            for (int i = lane; i < na; i += 64) {
                const int n = sh.act[i];
                best = fmax(best, (sh.hs[cur][0] + (double)sh.x[cur][n]) + (n == a.sil ? a.sil_score : 0.0));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, 64));
        if constexpr (LM) {
            if (lane == 0) sh.wmax[wave] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) best = fmax(best, sh.wmax[w]);
        }
        const double floor_ = best - a.thr;
        double rs = -INFINITY;
        uint32_t rc = DEAD;
        bool first = true;
        for (int base = wave * 64; base < NC; base += NTHREADS) {
            const int idx = base + lane;
            Key k = {-INFINITY, DEAD};
            if (idx < NC) {
                const int h = idx / na;
                k = eval_cand<LM>(sh, cur, h, sh.act[idx - h * na], floor_, a, lm);
            }
            if (!__ballot(k.c != DEAD)) continue;
            sort64(k.s, k.c, lane);
            if (first) {
                rs = k.s; rc = k.c;
                first = false;
                continue;
            }
            const double ts = __shfl(k.s, 63 - lane, 64);      // the batch's best 32, worst first, for the upper lanes
            const uint32_t tc = __shfl(k.c, 63 - lane, 64);
            merge32(rs, rc, ts, tc, lane);
        }
        if (lane < 32) { sh.top_s[wave][lane] = rs; sh.top_c[wave][lane] = rc; }
        __syncthreads();
        // ---- 3: the next beam
        if (wave == 0) {
            for (int w = 1; w < NWAVES; ++w) {
                const double ts = sh.top_s[w][(63 - lane) & 31];      // lane 32 + i reads entry 31 - i: worst first
                const uint32_t tc = sh.top_c[w][(63 - lane) & 31];
                if (__ballot(tc != DEAD)) merge32(rs, rc, ts, tc, lane);
            }
            const bool surv = lane < beam && rc != DEAD;
            const unsigned long long smask = __ballot(surv);
            const int h = surv ? (int)(rc >> 8) : 0, n = surv ? (int)(rc & 255u) : 0;
            const int oprev = sh.prev[cur][h], oflag = sh.flag[cur][h], ohist = sh.hist[cur][h], opar = sh.par[cur][h];
            const bool ext = surv && n != a.blank && (n != oprev || oflag);
            int id = -1, headv = -1;
            uint32_t bucket = 0xffffffffu;
            int nstate = 0;            // LM: the state of the survivor's history: kept, read from a known node, or next[state][n]
            if constexpr (LM) nstate = sh.lms[cur][h];
            if (ext) {
                bucket = node_hash(ohist, n) & hmask;
                headv = heads[bucket];
                for (id = headv; id >= 0;) {
                    const int4 nd = nodes[id];
                    if (nd.x == ohist && nd.y == n) {
                        if constexpr (LM) nstate = nd.w;
                        break;
                    }
                    id = nd.z;
                }
                if constexpr (LM) {
                    if (id < 0) nstate = lm.next[nstate * V + n];
                }
            }
            const bool alloc = ext && id < 0;
            const unsigned long long amask = __ballot(alloc);
            const int pool_n = sh.pool_n;
            if (alloc) id = pool_n + __popcll(amask & ((1ull << lane) - 1ull));
            if (amask) {   // new nodes of one bucket chain in lane order in front of the old head; the lowest lane writes the head
                int chain = headv;
                bool lowest = true;
                for (int j = BMAX - 1; j >= 0; --j) {
                    const uint32_t bj = __shfl(bucket, j, 64);
                    const int idj = __shfl(id, j, 64);
                    if (((amask >> j) & 1ull) && bj == bucket) {
                        if (j > lane) chain = idj;
                        if (j < lane) lowest = false;
                    }
                }
                if (alloc) {
                    nodes[id] = make_int4(ohist, n, chain, nstate);
                    if (lowest) heads[bucket] = id;
                }
            }
            if (surv) {
                sh.hs[nxt][lane] = rs;
                sh.hist[nxt][lane] = ext ? id : ohist;
                sh.par[nxt][lane] = ext ? ohist : opar;
                sh.prev[nxt][lane] = n;
                sh.flag[nxt][lane] = n == a.blank ? 1 : 0;
                if constexpr (LM) sh.lms[nxt][lane] = nstate;
                bp[(long)t * beam + lane] = (uint16_t)rc;
            }
            if (lane == 0) {
                sh.nh = __popcll(smask);
                sh.pool_n = pool_n + __popcll(amask);
            }
        }
        if (tid < V && t + 1 < Tb) sh.x[nxt][tid] = x_next;
        __syncthreads();
    }

    // ---- the closing silence: hypotheses of equal history merge, floor and cut once more, the nbest best are walked back
    if (wave == 0) {
        const int cur = Tb & 1, nh = sh.nh;
        // LM: every hypothesis takes lm_wfinal of its history's state first; the maximum is then any slot's
        double fin = 0.0, top = sh.hs[cur][0];
        if constexpr (LM) {
            top = -INFINITY;
            if (lane < nh) {
                fin = lm.wfinal[sh.lms[cur][lane]];
                top = sh.hs[cur][lane] + fin;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o, 64));
        }
        const double floor_ = top - a.thr;
        double rs = -INFINITY;
        uint32_t rc = DEAD;
        if (lane < nh) {
            const double sc = LM ? sh.hs[cur][lane] + fin : sh.hs[cur][lane];
            const int hh = sh.hist[cur][lane];
            int q = -1;
            for (int h = 0; h < nh; ++h)
                if (h != lane && sh.hist[cur][h] == hh) q = h;
            bool alive = sc >= floor_;
            double m = sc;
            if (alive && q >= 0) {
                const double sq = LM ? sh.hs[cur][q] + fin : sh.hs[cur][q];      // equal history, equal state, equal term
                if (sq >= floor_) {
                    if (sq > sc || (sq == sc && q < lane)) alive = false;
                    else if (a.log_add) m = logaddexp_ge(sc, sq);
                }
            }
            if (alive) { rs = m; rc = ((uint32_t)lane << 8) | (uint32_t)a.sil; }
        }
        sort64(rs, rc, lane);
        const int nf = __popcll(__ballot(lane < beam && rc != DEAD));
        const int n_hyp = nf < a.nbest ? nf : a.nbest;
        if (lane == 0) { sh.n_hyp = n_hyp; a.n_hyp[b] = n_hyp; }
        if (lane < a.nbest) {
            a.score[(long)b * a.nbest + lane] = lane < n_hyp ? rs : -INFINITY;
            if (lane < n_hyp) {
                uint8_t* row = rows + (long)lane * (a.T + 2);
                int s = (int)(rc >> 8);
                row[Tb + 1] = (uint8_t)a.sil;
                for (int t = Tb - 1; t >= 0; --t) {
                    const uint32_t e = bp[(long)t * beam + s];
                    row[t + 1] = (uint8_t)(e & 255u);
                    s = (int)(e >> 8);
                }
                row[0] = (uint8_t)a.sil;
            }
        }
    }
    __syncthreads();
    // ---- read-out: collapse repeats over the T_b + 2 row, drop blanks; the positions kept are the timesteps
    const int n_hyp = sh.n_hyp, len = Tb + 2;
    for (int j = wave; j < a.nbest; j += NWAVES) {
        int32_t* tok = a.tokens + ((long)b * a.nbest + j) * a.max_n;
        int32_t* ts = a.timesteps + ((long)b * a.nbest + j) * a.max_n;
        int off = 0;
        if (j < n_hyp) {
            const uint8_t* row = rows + (long)j * (a.T + 2);
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                int v = 0;
                bool keep = false;
                if (i < len) {
                    v = row[i];
                    keep = v != a.blank && (i == 0 || v != row[i - 1]);
                }
                const unsigned long long m = __ballot(keep);
                const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
                if (keep && pos < a.max_n) { tok[pos] = v; ts[pos] = i; }
                off += __popcll(m);
            }
        }
        for (int i = (off < a.max_n ? off : a.max_n) + lane; i < a.max_n; i += 64) { tok[i] = 0; ts[i] = 0; }
        if (lane == 0) a.n_tok[(long)b * a.nbest + j] = off;
    }
}

// workspace of one launch: nodes | hash heads | back-pointers | token rows, every part 16-byte aligned
struct BeamLayout { int64_t node_cap, n_heads, nodes, heads, bp, rows, total; };
BeamLayout beam_layout(int64_t B, int64_t T, int64_t beam, int64_t nbest) {
    BeamLayout l;
    l.node_cap = T * beam + 1;                 // the root and at most `beam` new histories per frame
    l.n_heads = 64;
    while (l.n_heads < l.node_cap) l.n_heads *= 2;
    auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
    l.nodes = 0;
    l.heads = l.nodes + B * l.node_cap * 16;
    l.bp = l.heads + up(B * l.n_heads * 4);
    l.rows = l.bp + up(B * T * beam * 2);
    l.total = l.rows + up(B * nbest * (T + 2));
    return l;
}

// both entry points: the checks they share, then the instantiation without (lm == nullptr) or with a language model
int beam_search(const char* who, const LmArgs* lm, const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens,
                int64_t B, int64_t T, int64_t V, int blank, int sil, int beam_size, int beam_size_token, double beam_threshold,
                int log_add, double sil_score, int nbest, int64_t max_n, void* workspace, int32_t* tokens, int32_t* timesteps,
                int32_t* n_tok, double* score, int32_t* n_hyp, void* stream) {
    APTAI_REQUIRE(logits && workspace && tokens && timesteps && n_tok && score && n_hyp, "%s: null pointer", who);
    APTAI_REQUIRE(B > 0 && T > 0 && V > 0 && V <= MAXV && ldl >= V && rows_per_b >= T && T < (1 << 24),
                  "%s: bad sizes (V=%ld, max %d)", who, (long)V, MAXV);
    APTAI_REQUIRE(blank >= 0 && blank < V && sil >= 0 && sil < V && blank != sil, "%s: blank / silence token out of range", who);
    APTAI_REQUIRE(beam_size >= 1 && beam_size <= BMAX, "%s: beam_size must be 1..%d (got %d)", who, BMAX, beam_size);
    APTAI_REQUIRE(beam_size_token >= 0, "%s: beam_size_token must be >= 0 (0 = all tokens)", who);
    APTAI_REQUIRE(beam_threshold >= 0.0, "%s: beam_threshold must be >= 0", who);   // also refuses NaN
    APTAI_REQUIRE(sil_score == sil_score, "%s: sil_score is NaN", who);
    APTAI_REQUIRE(nbest >= 1 && nbest <= beam_size, "%s: nbest must be 1..beam_size (got %d, beam_size %d)", who, nbest, beam_size);
    APTAI_REQUIRE(max_n >= 1 && max_n < (1ll << 31), "%s: bad max_n", who);
    APTAI_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const BeamLayout l = beam_layout(B, T, beam_size, nbest);
    BeamArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = logits; a.ldl = ldl; a.rows_per_b = rows_per_b; a.input_lens = input_lens;
    a.T = (int)T; a.V = (int)V; a.blank = blank; a.sil = sil; a.beam = beam_size;
    a.ktok = (beam_size_token == 0 || beam_size_token > V) ? (int)V : beam_size_token;
    a.log_add = log_add != 0; a.nbest = nbest; a.max_n = (int)max_n;
    a.thr = beam_threshold; a.sil_score = sil_score;
    a.nodes = (int4*)((char*)workspace + l.nodes);
    a.heads = (int*)((char*)workspace + l.heads);
    a.bp = (uint16_t*)((char*)workspace + l.bp);
    a.rows = (uint8_t*)((char*)workspace + l.rows);
    a.node_cap = l.node_cap; a.n_heads = l.n_heads;
    a.tokens = tokens; a.timesteps = timesteps; a.n_tok = n_tok; a.n_hyp = n_hyp; a.score = score;
    if (lm) {
        APTAI_LAUNCH(ctc_beam_kernel<true>, dim3((unsigned)B), dim3(NTHREADS), 0, (hipStream_t)stream, a, *lm);
    } else {
        APTAI_LAUNCH(ctc_beam_kernel<false>, dim3((unsigned)B), dim3(NTHREADS), 0, (hipStream_t)stream, a, LmArgs{});
    }
    APTAI_CHECK_LAUNCH("ctc_beam_kernel");
    return APTAI_OK;
}

}  // namespace

extern "C" int64_t aptai_ctc_beam_search_workspace_bytes(int64_t B, int64_t T, int64_t beam_size, int64_t nbest) {
    if (B <= 0 || T <= 0 || beam_size <= 0 || beam_size > BMAX || nbest <= 0 || nbest > beam_size) return 0;
    return beam_layout(B, T, beam_size, nbest).total;
}

extern "C" int aptai_ctc_beam_search(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B,
                                     int64_t T, int64_t V, int blank, int sil, int beam_size, int beam_size_token,
                                     double beam_threshold, int log_add, double sil_score, int nbest, int64_t max_n, void* workspace,
                                     int32_t* tokens, int32_t* timesteps, int32_t* n_tok, double* score, int32_t* n_hyp, void* stream) {
    return beam_search("aptai_ctc_beam_search", nullptr, logits, ldl, rows_per_b, input_lens, B, T, V, blank, sil, beam_size,
                       beam_size_token, beam_threshold, log_add, sil_score, nbest, max_n, workspace, tokens, timesteps, n_tok, score,
                       n_hyp, stream);
}

extern "C" int aptai_ctc_beam_search_lm(const float* logits, int64_t ldl, int64_t rows_per_b, const int32_t* input_lens, int64_t B,
                                        int64_t T, int64_t V, int blank, int sil, int beam_size, int beam_size_token,
                                        double beam_threshold, int log_add, double sil_score, int nbest, int64_t max_n,
                                        void* workspace, int32_t* tokens, int32_t* timesteps, int32_t* n_tok, double* score,
                                        int32_t* n_hyp, const double* lm_w, const int32_t* lm_next, const double* lm_wfinal,
                                        int64_t lm_states, int lm_start, void* stream) {
    const char* who = "aptai_ctc_beam_search_lm";
    APTAI_REQUIRE(lm_w && lm_next && lm_wfinal, "%s: null language model table", who);
    APTAI_REQUIRE(lm_states >= 1, "%s: lm_states must be >= 1 (got %ld)", who, (long)lm_states);
    APTAI_REQUIRE(lm_start >= 0 && lm_start < lm_states, "%s: lm_start %d outside [0, lm_states = %ld)", who, lm_start, (long)lm_states);
    APTAI_REQUIRE(V > 0 && lm_states <= (1ll << 24) / V, "%s: lm_states * V must not exceed 2^24 (lm_states %ld, V=%ld)", who,
                  (long)lm_states, (long)V);
    const LmArgs lm = {lm_w, lm_next, lm_wfinal, lm_start};
    return beam_search(who, &lm, logits, ldl, rows_per_b, input_lens, B, T, V, blank, sil, beam_size, beam_size_token, beam_threshold,
                       log_add, sil_score, nbest, max_n, workspace, tokens, timesteps, n_tok, score, n_hyp, stream);
}
