/*
 * ba.h -- C ABI of libba_hip.so, the MI355X-native batched OM(m)
 * Byzantine-agreement engine.
 *
 * The reference (mathiasplans/byzantine-agreement, /root/reference/ba.py) has no
 * FFI: its hot path is a set of in-process Python methods that the REPL calls
 * (ba.py:381 order, ba.py:386 wait_majority, ba.py:395 quorum, ba.py:399 clear)
 * plus the rpyc service surface between generals (Serv.exposed_*, ba.py:25-63).
 * Each entry point below names the reference interface it replaces.  The
 * ctypes binding a maintainer adds on the reference side is in INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns 0 (BA_OK) or a negative BA_E* code; no exception
 *     or C++ type crosses the ABI.  ba_last_error() gives a thread-local text.
 *   - Host-pointer entry points copy in/out over PCIe; *_device entry points
 *     take device pointers and a hipStream_t (as void*) and are asynchronous.
 *   - One ctx per host thread; a ctx is not thread-safe.  The library owns
 *     the device scratch it allocates inside the ctx (including the run
 *     counter reduction slots).  Calls of one ctx may be made on different
 *     streams: the library orders each call after the ctx's previous one
 *     (an event it records on the previous call's stream when the stream
 *     changes), except while the stream is capturing a graph -- a graph
 *     replay's ordering is the caller's.  So a stream that carried a call of
 *     a ctx must stay valid until that ctx's next call or ba_ctx_destroy.  Device
 *     buffers a captured graph holds stay valid until the ctx grows its
 *     scratch for a LARGER call: give a graph its own ctx.  Replays of graphs
 *     captured from one ctx must not run concurrently with each other or with
 *     an eager call of that ctx: they share the ctx's scratch, counter sink
 *     and persistent-kernel task counter (one replay at a time per ctx).
 *     Capture a ctx's calls only after an eager call of at least the same
 *     size on that ctx: growing scratch or the LEVELS cascade's fan-in
 *     counters allocates (and zeroes the counters on the call's stream),
 *     which a capturing stream cannot do.
 *
 * General indexing: the live generals sorted by id are
 * indexed 0..n-1; index 0 is the commander (lowest live id, ba.py:381 +
 * election ba.py:126-157); 1..n-1 are lieutenants.  n <= BA_MAX_GENERALS.
 */
#ifndef BA_H
#define BA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BA_ABI_VERSION 1
#define BA_MAX_GENERALS 32
#define BA_MAX_DEPTH 8
#define BA_NCOUNTERS 16

/* error codes */
#define BA_OK 0
#define BA_EINVAL (-1)     /* bad argument (n, m, modes, sizes, null pointer)   */
#define BA_ENOMEM (-2)     /* device or host allocation failed                  */
#define BA_EDEVICE (-3)    /* HIP runtime error / no device                     */
#define BA_ENOTSUP (-4)    /* combination not supported (e.g. table mode, m>1)  */
#define BA_ETOOBIG (-5)    /* tree too large for the requested engine          */
#define BA_EABORTED (-6)   /* communicator aborted (watchdog timeout or a rank's  */
                           /* transport failure): destroy it, create a new one  */

/* lie source for faulty senders (ba.py:45, ba.py:269: random.randint(0,1)) */
#define BA_LIE_PHILOX 0 /* Philox4x32-10 keyed by (seed; trial word, level, slot) */
#define BA_LIE_TABLE 1  /* coins supplied in ba.py's canonical draw order (m=1)   */

/* faulty-set source (ba.py:401-407 g-state <id> faulty) */
#define BA_FAULTY_GIVEN 0  /* faulty_mask[] supplied by the caller               */
#define BA_FAULTY_RANDOM 1 /* f ~ U{0..f}, uniform f-subset of the n generals    */
#define BA_FAULTY_EXACT 2  /* exactly f faulty, uniform f-subset                 */

/* commander order source (ba.py:367-381 actual-order <o>) */
#define BA_ORDER_GIVEN 0  /* order[] supplied by the caller                     */
#define BA_ORDER_RANDOM 1 /* Bernoulli(1/2) attack/retreat                      */
#define BA_ORDER_CONST 2  /* every trial uses order_value                       */

/* order / decision codes.  Any order other than "attack" is relayed as
 * non-attack (ba.py:163-167, 177-181); the commander's own tally keeps it as
 * "other" (ba.py:208-215). */
#define BA_RETREAT 0
#define BA_ATTACK 1
#define BA_OTHER 2     /* order code only: e.g. `actual-order foo`           */
#define BA_UNDEFINED 2 /* decision code: root tie (ba.py:194-195)            */

/* quorum outcome codes (ba.py:246-253) */
#define BA_Q_RETREAT 0
#define BA_Q_ATTACK 1
#define BA_Q_UNDETERMINED 2

/* engines */
#define BA_ENGINE_AUTO 0
#define BA_ENGINE_FUSED 1  /* whole tree per 64-trial word resident on-chip     */
#define BA_ENGINE_LEVELS 2 /* level-synchronous, bit-packed levels in HBM       */

typedef struct ba_params {
    uint32_t n;            /* live generals, 1..32                                */
    uint32_t m;            /* OM depth; ba.py is m=1.  Effective depth min(m,n-2)   */
    uint64_t seed;         /* Philox key for lies and synthetic inputs           */
    uint32_t lie_mode;     /* BA_LIE_*                                            */
    uint32_t faulty_mode;  /* BA_FAULTY_*                                         */
    uint32_t f;            /* RANDOM: max f;  EXACT: f                            */
    uint32_t order_mode;   /* BA_ORDER_*                                          */
    uint32_t order_value;  /* BA_ORDER_CONST: BA_RETREAT/BA_ATTACK/BA_OTHER       */
    uint32_t engine;       /* BA_ENGINE_*                                         */
    uint64_t first_trial;  /* global index of trial 0; multiple of 64.  The last
                              trial, first_trial + batch - 1, may not pass
                              2^64 - 1 (BA_EINVAL, every entry point): a run may
                              end exactly at 2^64, never wrap                    */
    uint32_t table_stride; /* BA_LIE_TABLE: uint32 words per trial in lie_table   */
    uint32_t reserved[5];
} ba_params;

/* Run counters (integer sums; identical for any sharding of the trials). */
#define BA_C_TRIALS 0          /* trials resolved                                   */
#define BA_C_AGREEMENT 1       /* IC1: all loyal lieutenants decided alike          */
#define BA_C_VALID_APPL 2      /* commander loyal (IC2 applicable)                   */
#define BA_C_VALIDITY 3        /* IC2: loyal commander => loyal lts decide its order */
#define BA_C_Q_RETREAT 4       /* quorum outcome counts (ba.py:246-253)              */
#define BA_C_Q_ATTACK 5
#define BA_C_Q_UNDETERMINED 6
#define BA_C_UNDEF_DECISIONS 7 /* lieutenant decisions == undefined (root ties)      */
#define BA_C_IN_BOUND 8        /* trials with f <= m_eff and n > 3 m_eff             */
#define BA_C_BOUND_VIOL 9      /* in-bound trials violating IC1 or IC2               */
#define BA_C_FAULTY_TOTAL 10   /* sum of f over trials                               */
#define BA_C_ATTACK_DECISIONS 11 /* lieutenant decisions == attack                   */
/* Slot 14 (BA_C_CHECK_MISMATCH = BA_C_HANDOFF_LOST): non-zero means the call's
 * results are INVALID.  Every build counts there a granule hand-off of the
 * LEVELS cascade that stayed stale past its bounded poll (2 s; never on a
 * correct run -- a launch starved by other work on the GPU, or preempted that
 * long), and the check build (environment BA_CASC_CHECK=1, read per call; a
 * test switch) also counts hand-off tag mismatches there.  ba_run_trials and
 * the multi-rank jobs (ba_run_trials_multi, ba_run_instance_split*_multi) read
 * it back and return BA_EDEVICE ("in-launch hand-off timed out") instead of
 * results.  Callers of the asynchronous device entries (ba_run_trials_device,
 * ba_root_from_split_votes_device) MUST check slot 14 of their counters after
 * synchronizing before trusting decisions, outcomes or counters (ba_amd/lib.py:
 * check_handoff).  After such an error the ctx stays usable (every eager launch
 * tags its hand-offs with a new epoch); a captured graph repeats its launch's
 * epoch, so a graph whose replay reported it must be captured again.
 * BA_TEST_GRANULE_TICKS (tests only, read per call) shrinks the poll bound
 * (s_memrealtime ticks, 100 MHz) so a launch times out.
 * The cascade's in-launch hand-offs between workgroups rest on gfx950 / ROCm 7.2
 * behaviour measured in MI355X_MICROARCH.md, not on the HIP memory model:
 * granules ({32-bit value half, 32-bit launch tag} in one aligned 8-byte sc1
 * store, read with sc1 loads and re-read until the tag matches: the guide's R2
 * form, observed untorn) for R_1 and, in CO launches, R_{me-2}; drained sc1
 * stores + a relaxed agent-scope counter add + sc1 loads (the guide's
 * valid-forms row 1) only in the one-launch cascade and the non-default wave
 * fan-in (BA_CASC_MTOP=0). The check build and its
 * tests (tests/test_gpu_cascade.py, part of the GPU suite) watch both.
 * Slot 15 is the multi-GPU entries' error flag (always 0 in returned counters). */
#define BA_C_CHECK_MISMATCH 14
#define BA_C_HANDOFF_LOST BA_C_CHECK_MISMATCH

typedef struct ba_counters {
    uint64_t v[BA_NCOUNTERS];
} ba_counters;

/* Per-trial outputs
 *   decisions[t] : uint64, bits [2(r-1), 2(r-1)+1] = decision code of lieutenant r
 *                  (BA_RETREAT / BA_ATTACK / BA_UNDEFINED), r = 1..n-1.
 *                  Replaces Process.majority of each lieutenant (ba.py:188-195).
 *   outcome[t]   : uint8, bits 0-1 quorum code (ba.py:225-255), bit 2 IC1,
 *                  bit 3 IC2 applicable, bit 4 IC2, bit 5 in-bound.
 * Per-trial inputs
 *   faulty_mask[t] : uint32, bit i = general i faulty (ba.py:73, 407)
 *   order[t]       : uint8 order code (ba.py:381 cmd[1])
 *   lie_table      : table_stride uint32 words per trial; bit c (word c/32, bit
 *                    c%32) is the c-th coin of ba.py's canonical draw order,
 *                    1 = "attack" (random.randint(0,1) == 0).
 *   poll_commander : uint32 per trial (BA_LIE_TABLE only, NULL = none): bit r set
 *                    means lieutenant r also polls the commander in its relay
 *                    round.  ba.py:171 skips only the port a lieutenant believes is
 *                    the primary's; after g-add/g-kill that port can be stale or -1
 *                    (ba.py:86-102, 114-115), so the commander's answer is counted
 *                    too.  The stride must hold (n-1) + (n-1)^2 coins.
 */

/* ---- library / context (replaces Process/Serv lifecycle, ba.py:66-112) ---- */
int ba_version(void);
int ba_device_count(int* count);
int ba_ctx_create(int device, struct ba_ctx** out);
void ba_ctx_destroy(struct ba_ctx* ctx);
const char* ba_last_error(void);

/* ---- the hot path -------------------------------------------------------
 * One call resolves `batch` independent OM(m) trials: commander send
 * (Process.order, ba.py:257-285), the relay tree with the lie rule
 * (Serv.exposed_get_order, ba.py:42-57), the recursive majority
 * (Process.get_majority, ba.py:159-195) and the quorum epilogue
 * (get_majorities + quorum, ba.py:197-255).  Null optional pointers:
 * faulty_mask (unless BA_FAULTY_GIVEN), order (unless BA_ORDER_GIVEN),
 * lie_table (unless BA_LIE_TABLE), decisions, outcome, counters.
 * Counters are OVERWRITTEN with this call's totals.
 */
int ba_run_trials(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                  const uint32_t* faulty_mask, const uint8_t* order,
                  const uint32_t* lie_table, const uint32_t* poll_commander,
                  uint64_t* decisions, uint8_t* outcome, ba_counters* counters);

/* Same computation on device buffers, enqueued on `stream` (a hipStream_t as
 * void*; NULL is HIP's null stream, as in every HIP API -- NOT the ctx stream,
 * which only the host-pointer entry point uses).  d_counters (BA_NCOUNTERS uint64 on device) is ACCUMULATED
 * into, so repeated calls sum; zero it first for one call's totals. */
int ba_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                         const uint32_t* d_faulty_mask, const uint8_t* d_order,
                         const uint32_t* d_lie_table, const uint32_t* d_poll_commander,
                         uint64_t* d_decisions, uint8_t* d_outcome, uint64_t* d_counters,
                         void* stream);

/* Synthetic inputs of trials [p->first_trial, p->first_trial + batch): the
 * faulty sets (p->faulty_mode RANDOM or EXACT) and commander orders
 * (p->order_mode RANDOM or CONST) that ba_run_trials_device would otherwise
 * draw itself -- the same Philox stream, so running the batch on these as
 * BA_FAULTY_GIVEN / BA_ORDER_GIVEN inputs gives bit-identical results.  This
 * stages a workload's per-trial inputs in HBM ahead of time (bench.py does so
 * before its timed region; the lies stay inside the run: they are the faulty
 * generals' coin flips during the protocol, ba.py:45, 269).  Either output may
 * be NULL; a non-NULL one whose mode is GIVEN is BA_EINVAL.  Asynchronous on
 * `stream` (NULL = HIP's null stream). */
int ba_gen_inputs_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                         uint32_t* d_faulty_mask, uint8_t* d_order, void* stream);

/* ---- SM(m): signed messages ------------------------------------------------
 * Lamport, Shostak and Pease's other algorithm (no ba.py analogue: ba.py's
 * messages are oral).  Signatures cannot be forged, so SM(m) copes with any
 * f <= m traitors for any n, where OM(m) needs n > 3m.  One call resolves `batch`
 * independent trials in the synchronous-round form of docs/SEMANTICS.md §6:
 *   round 0      the commander signs and sends its order; a faulty commander
 *                signs either value, each by a coin per lieutenant (§6 "Round 0");
 *   accept       a lieutenant adds a received value it does not hold to its set
 *                V, and the value is fresh for it next round (§6 "Accept");
 *   rounds 1..me every lieutenant relays its fresh values with its signature
 *                added, a loyal one to all, a faulty one by a coin per recipient
 *                (§6 "Round k"); me = min(m, n-2);
 *   decision     choice(V): V = {attack} -> attack, anything else -> retreat
 *                (§6 "Decision"), then ba.py's quorum and the IC1/IC2 flags
 *                (§6 "Epilogue"), with in-bound meaning |F| <= m.
 * Coins are coin(64 + k, x) of the OM lie stream (§6 "Coins"); the synthetic
 * inputs are ba_run_trials' own (§6 "Synthetic inputs"), so an OM and an SM run
 * with equal params see the same faulty sets and orders.  decisions / outcome /
 * counters: the layouts above; BA_C_UNDEF_DECISIONS is always 0 and
 * BA_C_IN_BOUND / BA_C_BOUND_VIOL follow the SM bound.
 */

/* Lamport's SM(m) (signed messages); docs/SEMANTICS.md §6.  p->lie_mode must be
 * BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO (else BA_EINVAL);
 * every faulty/order mode, first_trial and seed as in ba_run_trials.
 * vsets[t] (optional): bit 2(r-1) = attack in V_r, bit 2(r-1)+1 = retreat in V_r.
 * Both bits set is lieutenant r's proof that the commander signed two orders. */
int ba_sm_run_trials(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                     const uint32_t* faulty_mask, const uint8_t* order,
                     uint64_t* decisions, uint8_t* outcome, uint64_t* vsets,
                     ba_counters* counters);              /* counters overwritten */
/* The same rounds (§6 "Round 0" .. "Epilogue") on device buffers, enqueued on
 * `stream` in the ctx's call order (NULL = HIP's null stream). */
int ba_sm_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                            const uint32_t* d_faulty_mask, const uint8_t* d_order,
                            uint64_t* d_decisions, uint8_t* d_outcome, uint64_t* d_vsets,
                            uint64_t* d_counters, void* stream);  /* accumulated, async */
/* §6 "Coins": L + me L (L-1), L = n-1 -- one call per lieutenant in round 0 and
 * one per (sender, recipient) pair in each relay round (0 for n outside 1..32
 * or m > 8). */
uint64_t ba_sm_coin_calls(uint32_t n, uint32_t m);   /* Philox calls per 64-trial word; host only */

/* ---- OM(m) against scripted traitors ------------------------------------------
 * ba_run_trials' traitors flip a fair coin per message; these entries replace
 * the coin by a deterministic policy (docs/SEMANTICS.md §7), which is how
 * Lamport, Shostak and Pease argue: with n <= 3m a traitor that chooses its
 * messages breaks OM(m), with n > 3m no choice does.  Everything but the lie
 * rule is ba_run_trials': effective depth, majorities, root tie -> undefined,
 * quorum, flags, the in-bound rule and the synthetic inputs (an OM and an ADV
 * run with equal params see the same faulty sets and orders).  A faulty sender
 * (the commander at level 0, else the path's last lieutenant) shows recipient
 * rank j, in place of the truth T it holds:
 *   BA_ADV_SPLIT  attack to odd ranks, retreat to even ones, at every level
 *                 (the paper's two-faced traitor);
 *   BA_ADV_FLIP   1 - T;
 *   BA_ADV_ANTI   level 0 as SPLIT; deeper, the opposite of what j itself got
 *                 from the commander (aims at ties).
 * No coin is drawn: results depend on (n, m, policy, faulty set, order) only, and
 * on seed / first_trial only through the synthetic inputs.  p->lie_mode must be
 * BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO (else BA_EINVAL),
 * policy <= BA_ADV_ANTI (else BA_EINVAL).  A receiver walks its ba_adv_paths(n, m)
 * relay chains one by one; above 2^24 of them the call is BA_ETOOBIG ((16,6),
 * (32,4), (12,8) fit; (32,5), (16,7), (16,8) do not).  decisions / outcome /
 * counters: the OM layouts above. */
#define BA_ADV_SPLIT 0
#define BA_ADV_FLIP 1
#define BA_ADV_ANTI 2
int ba_adv_run_trials(struct ba_ctx* ctx, const ba_params* p, uint32_t policy, uint64_t batch,
                      const uint32_t* faulty_mask, const uint8_t* order, uint64_t* decisions,
                      uint8_t* outcome, ba_counters* counters);  /* counters overwritten */
/* The same walk on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream). */
int ba_adv_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint32_t policy,
                             uint64_t batch, const uint32_t* d_faulty_mask,
                             const uint8_t* d_order, uint64_t* d_decisions, uint8_t* d_outcome,
                             uint64_t* d_counters, void* stream);  /* accumulated, async */
/* P(n-2, me): the leaf chains one receiver resolves (§7); 1 when me = 0, and 0 for
 * n outside 1..32 or m > 8. */
uint64_t ba_adv_paths(uint32_t n, uint32_t m);   /* host only */

/* ---- OM(m) against every traitor strategy of one case ---------------------------
 * A policy is one adversary; Lamport's theorem speaks of every choice of messages.
 * These entries walk all of them for one case (n, m, faulty set, order)
 * (docs/SEMANTICS.md §8; no ba.py analogue).  Every message a traitor sends to a
 * LOYAL lieutenant is a free bit; a message between two traitors is retreat (it
 * cannot change a loyal lieutenant's decision, §8); a loyal sender relays the
 * truth.  A strategy S is an assignment of the B = ba_enum_bits(n, m, faulty_mask)
 * free bits: bit i of S is the value of the i-th free slot in (level ascending,
 * lexicographic path rank ascending) order, 1 = attack (ba_enum_slots lists them).
 * Trial t of a call is strategy S = t: a call covers S in [p->first_trial,
 * p->first_trial + batch), first_trial a multiple of 64, ending at or below 2^B
 * (else BA_EINVAL).  p supplies n, m and first_trial; seed and f are unused.
 * p->lie_mode must be BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO,
 * p->faulty_mode BA_FAULTY_GIVEN and p->order_mode BA_ORDER_GIVEN (else BA_EINVAL):
 * the one faulty_mask (masked to n bits) and the one order code (<= BA_OTHER, else
 * BA_EINVAL) of all the call's trials are arguments.  B > BA_ENUM_MAX_BITS and
 * ba_tree_slots(n, m) > 4096 are BA_ETOOBIG.  decisions / outcome / counters: the
 * OM layouts above, faulty lieutenants deciding on their dead slots at retreat.
 * witness: the smallest S of the range that violates IC1 or (IC2 applicable) IC2,
 * in bound or not, or 2^64 - 1 when none does.  batch = 0: BA_OK, zero counters,
 * witness 2^64 - 1.  Every call copies the case's slot map (at most 4 KiB) from
 * pageable host memory to the device on the call's stream.  The HIP runtime finishes
 * such a copy before it returns, so ba_enum_run_device is NOT fully asynchronous: it
 * returns after the stream's earlier work has drained and the map has landed, with
 * its own launches queued behind.  For the same reason ba_enum_run_device on a stream
 * that is capturing a graph is refused with BA_ENOTSUP, before anything is queued on
 * the stream: the capture stays valid.  (ba_enum_run plans the case and copies the map once, whatever the
 * number of its output chunks.) */
#define BA_ENUM_MAX_BITS 48
/* B; host only.  0xFFFFFFFF for n outside 1..32 or m > 8; saturates at 0xFFFFFFFE. */
uint32_t ba_enum_bits(uint32_t n, uint32_t m, uint32_t faulty_mask);
/* bit i -> (level[i], slot[i] = path rank in that level); host only.  Returns B, or
 * BA_EINVAL (bad n / m, cap < B), BA_ETOOBIG (the two caps). */
int ba_enum_slots(uint32_t n, uint32_t m, uint32_t faulty_mask, uint32_t* level, uint64_t* slot,
                  uint32_t cap);
int ba_enum_run(struct ba_ctx* ctx, const ba_params* p, uint32_t faulty_mask, uint32_t order,
                uint64_t batch, uint64_t* decisions, uint8_t* outcome, ba_counters* counters,
                uint64_t* witness);  /* counters and witness overwritten */
/* The same walk on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream).  d_counters is accumulated into; d_witness (optional)
 * is min-accumulated: the caller sets it to 2^64 - 1 first.  The launches are
 * asynchronous; the call itself waits for the stream's earlier work (the map copy,
 * above). */
int ba_enum_run_device(struct ba_ctx* ctx, const ba_params* p, uint32_t faulty_mask,
                       uint32_t order, uint64_t batch, uint64_t* d_decisions, uint8_t* d_outcome,
                       uint64_t* d_counters, uint64_t* d_witness, void* stream);

/* ---- Phase King: unsigned, polynomial ------------------------------------------
 * Berman, Garay and Perry's protocol (docs/SEMANTICS.md §9; no ba.py analogue): oral
 * messages like OM(m), but (m+1) n^2 one-bit messages where OM's relay tree has
 * P(n-1, m+1) leaves, at the price of the bound n > 4m.  Every general, the
 * commander included, keeps one preference bit and runs the rules honestly; being
 * faulty only replaces what a general sends.
 *   round 0      the commander sends its order; each lieutenant's preference is
 *                what it was shown, the commander's its order bit;
 *   phase p      p = 1..P, P = ba_king_phases(n, m) = min(m, n-1) + 1, king = general
 *                p-1.  Exchange: everyone sends its preference to everyone; general i
 *                counts the attack votes c1 of all n generals (its own true value
 *                included), maj = [2 c1 > n], mult = the majority's count, strong =
 *                [2 mult > n + 2m] (the parameter m).  King: the king sends its maj;
 *                i keeps maj if strong, else takes the king's value (the king its own);
 *   decision     lieutenant r decides its preference after phase P (never undefined),
 *                then ba.py's quorum and the IC1/IC2 flags over the commander's order
 *                and the lieutenants' decisions, as everywhere else.
 * A faulty sender j shows recipient r, in place of the truth, under
 *   BA_KING_COIN   the coin c(q, 32 j + r) = coin(128 + q, 32 j + r) of the OM lie
 *                  stream, q = 0 the commander's send, 2p-1 / 2p phase p's rounds;
 *   BA_KING_SPLIT  r & 1: attack to odd general indices, retreat to even ones, in
 *                  every round (no coin is drawn).
 * Neither is the worst case: rates beyond the bound are rates against these two.
 * In-bound means |F| <= m and n > 4m (BA_C_IN_BOUND / BA_C_BOUND_VIOL follow it);
 * BA_C_UNDEF_DECISIONS is always 0.  The synthetic inputs are ba_run_trials' own: an
 * OM, SM and KING run with equal params see the same faulty sets and orders.
 * p->lie_mode must be BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO,
 * policy <= BA_KING_SPLIT (else BA_EINVAL); every faulty/order mode, first_trial and
 * seed as in ba_run_trials.  decisions / outcome / counters: the layouts above.
 * settled[t] (optional, uint8): the smallest p in 0..P such that all loyal generals
 * (a loyal commander included) hold one common preference at the end of phase p and
 * of every later phase (phase 0 = round 0; none or one loyal general agrees), or 255
 * if they differ after phase P. */
#define BA_KING_COIN 0
#define BA_KING_SPLIT 1
int ba_king_run_trials(struct ba_ctx* ctx, const ba_params* p, uint32_t policy, uint64_t batch,
                       const uint32_t* faulty_mask, const uint8_t* order, uint64_t* decisions,
                       uint8_t* outcome, uint8_t* settled,
                       ba_counters* counters);             /* counters overwritten */
/* The same rounds on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream). */
int ba_king_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint32_t policy,
                              uint64_t batch, const uint32_t* d_faulty_mask,
                              const uint8_t* d_order, uint64_t* d_decisions, uint8_t* d_outcome,
                              uint8_t* d_settled, uint64_t* d_counters,
                              void* stream);               /* accumulated, async */
/* ceil(n/2) (1 + P (n+1)): Philox calls per 64-trial word when every sender is faulty
 * somewhere in the word (one call serves recipients r and r ^ 1 of one sender).  0 for
 * n outside 1..32 or m > 8. */
uint64_t ba_king_coin_calls(uint32_t n, uint32_t m);   /* host only */
/* P = min(m, n-1) + 1; 0 for n outside 1..32 or m > 8. */
uint32_t ba_king_phases(uint32_t n, uint32_t m);       /* host only */

/* ---- KING3: the three-round King algorithm, unsigned, polynomial, n > 3m -------
 * Berman, Garay and Perry's second algorithm (docs/SEMANTICS.md §10; no ba.py
 * analogue): Phase King's setting, participants, faulty stance, adversaries and
 * outputs, but three rounds per phase, about 2n^2 + n messages, and agreement
 * whenever n > 3m, the optimal resilience that OM(m) pays for with its relay tree.
 *   round 0      as Phase King's;
 *   phase p      p = 1..P, P = ba_king3_phases(n, m) = min(m, n-1) + 1, king = general
 *                p-1.  All thresholds use the parameter m and compare signed integers
 *                (n - m <= 0 always holds).
 *                Value: everyone sends its preference; general i counts the attack
 *                votes c1 of all n generals (its own true value included), c0 = n - c1,
 *                and will propose retreat if c0 >= n-m, else attack if c1 >= n-m, else
 *                nothing.  Propose: everyone shows its proposal (a faulty sender always
 *                proposes); i counts d0 and d1, x = retreat if d0 > m, else attack if
 *                d1 > m, else its preference; sure = [d_x >= n-m].  King: the king
 *                sends its x; i keeps x if sure, else takes the king's value (the king
 *                its own);
 *   decision     as Phase King's.
 * A faulty sender j shows recipient r, in place of the truth, under
 *   BA_KING_COIN   the coin c(q, 32 j + r) = coin(192 + q, 32 j + r), q = 0 the
 *                  commander's send, 3p-2 / 3p-1 / 3p phase p's rounds;
 *   BA_KING_SPLIT  r & 1 in every round (no coin is drawn).
 * Neither is the worst case: rates beyond the bound are rates against these two.
 * In-bound means |F| <= m and n > 3m.  p->m <= 10 at these entries (32 > 3 * 10; every
 * other entry keeps BA_MAX_DEPTH), else BA_EINVAL; p->lie_mode must be BA_LIE_PHILOX
 * (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO, policy <= BA_KING_SPLIT (else
 * BA_EINVAL); every faulty/order mode, first_trial and seed as in ba_run_trials, and
 * the synthetic inputs are ba_run_trials' own.  decisions / outcome / counters /
 * settled: as ba_king_run_trials. */
int ba_king3_run_trials(struct ba_ctx* ctx, const ba_params* p, uint32_t policy, uint64_t batch,
                        const uint32_t* faulty_mask, const uint8_t* order, uint64_t* decisions,
                        uint8_t* outcome, uint8_t* settled,
                        ba_counters* counters);            /* counters overwritten */
/* The same rounds on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream). */
int ba_king3_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint32_t policy,
                               uint64_t batch, const uint32_t* d_faulty_mask,
                               const uint8_t* d_order, uint64_t* d_decisions, uint8_t* d_outcome,
                               uint8_t* d_settled, uint64_t* d_counters,
                               void* stream);              /* accumulated, async */
/* ceil(n/2) (1 + P (2n+1)): Philox calls per 64-trial word when every sender is faulty
 * somewhere in the word.  0 for n outside 1..32 or m > 10. */
uint64_t ba_king3_coin_calls(uint32_t n, uint32_t m);  /* host only */
/* P = min(m, n-1) + 1; 0 for n outside 1..32 or m > 10. */
uint32_t ba_king3_phases(uint32_t n, uint32_t m);      /* host only */

/* ---- RAND: randomized agreement, Ben-Or rounds with a local or a common coin -----
 * Ben-Or's protocol in Bracha's threshold form (docs/SEMANTICS.md §13; no ba.py
 * analogue): KING3's setting, participants, faulty stance, adversaries and epilogue,
 * no king, R phases chosen by the caller (1..BA_RAND_MAX_PHASES), and agreement with
 * probability 1 rather than after m+1 phases.  Every general also keeps a sticky
 * flag D ("decided") and the value V it decided.
 *   round 0      as Phase King's;
 *   phase p      Report (q = 3p-2): everyone sends its preference x; general i counts
 *                the attack votes c1 of all n generals (its own true value included),
 *                c0 = n - c1, and will propose attack if 2 c1 > n+m, else retreat if
 *                2 c0 > n+m, else nothing.  Propose (q = 3p-1): everyone shows its
 *                proposal (a faulty sender always shows a value); i counts d0 and d1,
 *                v = retreat if d0 > m, else attack if d1 > m, else none; where v
 *                exists x = v, and if also 2 d_v > n+m and D is clear, D = 1, V = v.
 *                Toss (q = 3p): where v is none, x = i's coin of the phase:
 *                BA_RAND_LOCAL its own c(3p, 33 i), BA_RAND_COMMON the one coin
 *                c(3p, 0) of the trial, an ideal common coin the protocol assumes;
 *   decision     lieutenant r decides its x after phase R (never undefined), then the
 *                quorum and the IC1/IC2 flags as everywhere else.
 * A faulty sender j shows recipient r != j, in rounds 0, 3p-2 and 3p-1, under
 *   BA_KING_COIN   c(q, 32 j + r), where c(q, x) = coin(256 + q, x) of the OM lie stream;
 *   BA_KING_SPLIT  r & 1 (no message coin is drawn; the tosses still are).
 * Neither sees the coin, neither is the worst case.  In-bound means |F| <= m and
 * n > 3m.  BA_C_BOUND_VIOL therefore counts in-bound trials still split (or invalid)
 * after R phases: non-termination within R, which has a probability, not a safety
 * failure.  Safety is what decided[t] (optional, uint8) reports, by precedence:
 *   BA_RAND_UNSAFE     at the end of some phase two loyal generals with D set held
 *                      different V, or a loyal general with D set had x != V, or the
 *                      commander was loyal and a loyal general's V was not its order;
 *   p in 1..R          the first phase at whose end every loyal general (a loyal
 *                      commander included) has D set; 1 when nobody is loyal;
 *   BA_RAND_UNDECIDED  neither.
 * In bound BA_RAND_UNSAFE never appears.  p->m <= 10, p->lie_mode BA_LIE_PHILOX (TABLE:
 * BA_ENOTSUP), p->engine BA_ENGINE_AUTO, policy <= BA_KING_SPLIT, coin <=
 * BA_RAND_COMMON, phases in 1..BA_RAND_MAX_PHASES (else BA_EINVAL); every faulty/order
 * mode, first_trial and seed as in ba_run_trials, and the synthetic inputs are
 * ba_run_trials' own.  decisions / outcome / counters: the layouts above. */
#define BA_RAND_LOCAL 0
#define BA_RAND_COMMON 1
#define BA_RAND_MAX_PHASES 64
#define BA_RAND_UNDECIDED 255
#define BA_RAND_UNSAFE 254
int ba_rand_run_trials(struct ba_ctx* ctx, const ba_params* p, uint32_t policy, uint32_t coin,
                       uint32_t phases, uint64_t batch, const uint32_t* faulty_mask,
                       const uint8_t* order, uint64_t* decisions, uint8_t* outcome,
                       uint8_t* decided, ba_counters* counters);   /* counters overwritten */
/* The same phases on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream). */
int ba_rand_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint32_t policy,
                              uint32_t coin, uint32_t phases, uint64_t batch,
                              const uint32_t* d_faulty_mask, const uint8_t* d_order,
                              uint64_t* d_decisions, uint8_t* d_outcome, uint8_t* d_decided,
                              uint64_t* d_counters, void* stream);   /* accumulated, async */
/* ceil(n/2) (1 + 2 n R) + R (LOCAL ? n : 1): Philox calls per 64-trial word when every
 * sender is faulty somewhere in the word and every toss is drawn.  0 for n outside
 * 1..32, phases outside 1..64 or coin > 1. */
uint64_t ba_rand_coin_calls(uint32_t n, uint32_t phases, uint32_t coin);  /* host only */

/* ---- RAND against a stalling adversary that sees the loyal state ----------------
 * RAND's rules, tosses, decided byte, epilogue and in-bound rule above, unchanged
 * (docs/SEMANTICS.md §15; no ba.py analogue); only what a faulty sender shows differs,
 * and no message coin is drawn.  With F the faulty set, f = |F| and rank(j) the number
 * of faulty generals below j:
 *   round 0      a faulty commander shows a loyal lieutenant r the bit r & 1 and a
 *                faulty one retreat;
 *   report       with a the number of loyal generals whose x is attack at the start of
 *                the phase and t = min(max(floor(n/2) - a, 0), f), a faulty j shows
 *                every loyal general attack iff rank(j) < t, and a faulty one retreat:
 *                every loyal general counts c1 = a + t, as near floor(n/2) as can be;
 *   propose      with P1 and P0 the loyal generals that propose attack and retreat, a
 *                faulty j shows every loyal general retreat if P1 > P0, else attack,
 *                and a faulty one no proposal.
 * The adversary reads x after the previous phase's toss, which is all a synchronous
 * adversary can see before it speaks; it does not rush the coin within a phase, and it
 * is no worst case for safety.  In bound it keeps local coins undecided until all loyal
 * tosses of a phase fall alike, and costs the common coin one phase.
 * Arguments and errors are ba_rand_run_trials' without the policy: p->m <= 10,
 * p->lie_mode BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO, coin <=
 * BA_RAND_COMMON, phases in 1..BA_RSTALL_MAX_PHASES (else BA_EINVAL). */
#define BA_RSTALL_MAX_PHASES 250
int ba_rstall_run_trials(struct ba_ctx* ctx, const ba_params* p, uint32_t coin, uint32_t phases,
                         uint64_t batch, const uint32_t* faulty_mask, const uint8_t* order,
                         uint64_t* decisions, uint8_t* outcome, uint8_t* decided,
                         ba_counters* counters);   /* counters overwritten */
/* The same phases on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream). */
int ba_rstall_run_trials_device(struct ba_ctx* ctx, const ba_params* p, uint32_t coin,
                                uint32_t phases, uint64_t batch, const uint32_t* d_faulty_mask,
                                const uint8_t* d_order, uint64_t* d_decisions, uint8_t* d_outcome,
                                uint8_t* d_decided, uint64_t* d_counters,
                                void* stream);   /* accumulated, async */
/* R (LOCAL ? n : 1): Philox calls per 64-trial word when every toss is drawn.  0 for n
 * outside 1..32, phases outside 1..250 or coin > 1. */
uint64_t ba_rstall_coin_calls(uint32_t n, uint32_t phases, uint32_t coin);  /* host only */

/* ---- Phase King and KING3 against every traitor strategy of one case -----------
 * BA_KING_COIN and BA_KING_SPLIT are two adversaries; the theorems (agreement whenever
 * n > 4m, n > 3m) speak of every choice of messages.  These entries walk all of them
 * for one case (proto, n, m, faulty set, order) (docs/SEMANTICS.md §11; no ba.py
 * analogue), as the ba_enum entries do for OM(m).  proto is BA_KENUM_KING (the
 * rules of Phase King above) or BA_KENUM_KING3 (those of KING3); every general,
 * faulty ones included, keeps a preference and runs the rules honestly.  A message
 * from sender j to recipient i != j in round q (q = 0 the commander's send; Phase
 * King: 2p-1 exchange, 2p king; KING3: 3p-2 value, 3p-1 propose, 3p king) is
 *   truth   j is loyal;
 *   dead    j and i are both faulty: retreat, and no proposal in KING3's propose
 *           round (it cannot reach a loyal general's state);
 *   free    j is faulty, i loyal: one free bit, 1 = attack; in KING3's propose round
 *           two consecutive bits (lo, hi): lo = 0 is no proposal whatever hi is,
 *           lo = 1 proposes hi.  A traitor may thus withhold a proposal, which the
 *           coin and split adversaries never do; the codes (0,0) and (0,1) are one
 *           strategy, so rates are rates over the coded space.
 * Free bits are numbered in (q, sender, recipient) ascending order, lo before hi
 * (ba_kenum_slots lists them).  With l = n - |F|, P the protocol's phase count and
 * fK the faulty generals among the kings 0..P-1:
 *   B = [0 in F] l + P |F| l + fK l      (BA_KENUM_KING)
 *   B = [0 in F] l + 3 P |F| l + fK l    (BA_KENUM_KING3)
 * Trial t of a call is strategy S = t: a call covers S in [p->first_trial,
 * p->first_trial + batch), first_trial a multiple of 64, ending at or below 2^B
 * (else BA_EINVAL).  p supplies n, m and first_trial; seed and f are unused.
 * p->lie_mode must be BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO,
 * p->faulty_mode BA_FAULTY_GIVEN and p->order_mode BA_ORDER_GIVEN (else BA_EINVAL);
 * proto > 1, order > BA_OTHER, m > 8 (KING) and m > 10 (KING3) are BA_EINVAL.
 * B > BA_ENUM_MAX_BITS and n > 16 are BA_ETOOBIG: the kernel keeps one plane per
 * general in registers and is built for n = 1..16.  The 48-bit cap already excludes
 * nearly every larger case; what the n cap loses beyond it, all with n in 17..32:
 * no traitor at all (B = 0); Phase King with m = 0 and up to three traitors (n <= 32,
 * 26, 19 for one, two, three), m = 1 and one traitor (n <= 25), m = 2 and one
 * traitor at n = 17; KING3 with m = 0 and one traitor at n = 17.
 * decisions / outcome / counters: the layouts above, each protocol's own in-bound
 * rule, faulty lieutenants deciding honestly on truth and dead inputs.  witness: the
 * smallest S of the range that violates IC1 or (IC2 applicable) IC2, in bound or
 * not, or 2^64 - 1 when none does.  batch = 0: BA_OK, zero counters, witness
 * 2^64 - 1.  At most 2^40 strategies go into one launch.  Nothing is copied from
 * host memory: ba_kenum_run_device is fully asynchronous and may be captured in a
 * graph. */
#define BA_KENUM_KING 0
#define BA_KENUM_KING3 1
/* B; host only.  0xFFFFFFFF for proto > 1, n outside 1..32 or m above the
 * protocol's limit; saturates at 0xFFFFFFFE.  Not limited to n <= 16. */
uint32_t ba_kenum_bits(uint32_t proto, uint32_t n, uint32_t m, uint32_t faulty_mask);
/* bit i -> the message (q[i], sender[i] -> recipient[i]) and part[i]: 0 for a one-bit
 * message, 0 / 1 for lo / hi of a proposal; host only.  Returns B, or BA_EINVAL
 * (0xFFFFFFFF as uint32: a bad proto / n / m, cap < B, a missing array). */
int ba_kenum_slots(uint32_t proto, uint32_t n, uint32_t m, uint32_t faulty_mask, uint32_t* q,
                   uint32_t* sender, uint32_t* recipient, uint32_t* part, uint32_t cap);
int ba_kenum_run(struct ba_ctx* ctx, const ba_params* p, uint32_t proto, uint32_t faulty_mask,
                 uint32_t order, uint64_t batch, uint64_t* decisions, uint8_t* outcome,
                 ba_counters* counters, uint64_t* witness);  /* counters and witness overwritten */
/* The same walk on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream).  d_counters is accumulated into; d_witness (optional)
 * is min-accumulated: the caller sets it to 2^64 - 1 first. */
int ba_kenum_run_device(struct ba_ctx* ctx, const ba_params* p, uint32_t proto,
                        uint32_t faulty_mask, uint32_t order, uint64_t batch,
                        uint64_t* d_decisions, uint8_t* d_outcome, uint64_t* d_counters,
                        uint64_t* d_witness, void* stream);  /* accumulated, async */

/* ---- SM(m) against every strategy of a traitor coalition ------------------------
 * ba_sm_run_trials' traitors flip coins, relay only what they accepted a round ago
 * and share nothing; Lamport's theorem (agreement for any f <= m, any n) speaks of
 * traitors that pool their signatures and pick their messages.  These entries walk
 * every such strategy of one case (form, n, m, faulty set, order) (docs/SEMANTICS.md
 * §12; no ba.py analogue).  With me = min(m, n-2), c = [0 in F], l loyal and fL
 * faulty lieutenants and K = min(me, fL): in round k = 1..K any faulty lieutenant can
 * deliver a validly signed value to a loyal one whatever went before -- either value
 * when the commander is faulty, the order's value alone when it is loyal.  Later
 * rounds would need a loyal signature, which exists only on values every loyal
 * lieutenant was shown already: such messages change nothing and are not coded.
 * A free bit is one such message, 1 = sent:
 *   BA_SMENUM_MESSAGES   bits in (k, sender, recipient, v) ascending order, retreat
 *                        before attack; round 0 (the faulty commander's) first:
 *                          B = c 2l + K fL l (1 + c)
 *   BA_SMENUM_COALITION  a recipient accepts from any sender, so one bit per
 *                        (k, recipient, v): "some traitor delivers v in round k":
 *                          B = c 2l + K l (1 + c)
 *                        A message-form strategy and its projection (OR over the
 *                        senders) decide alike.  Rates are over the coded space of
 *                        the form used.
 * Loyal generals follow SM(m); faulty lieutenants keep V honestly on what loyal
 * senders show them (one V for all of them) and decide choice(V).
 * Trial t of a call is strategy S = t: a call covers S in [p->first_trial,
 * p->first_trial + batch), first_trial a multiple of 64, ending at or below 2^B
 * (else BA_EINVAL).  p supplies n, m and first_trial; seed and f are unused.
 * p->lie_mode must be BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine BA_ENGINE_AUTO,
 * p->faulty_mode BA_FAULTY_GIVEN and p->order_mode BA_ORDER_GIVEN (else BA_EINVAL);
 * form > 1, order > BA_OTHER, m > 8 and n outside 1..32 are BA_EINVAL.
 * B > BA_ENUM_MAX_BITS is BA_ETOOBIG; every n <= 32 is accepted.
 * decisions / outcome / counters: the layouts above, in-bound is |F| <= m.  witness:
 * the smallest S of the range that violates IC1 or (IC2 applicable) IC2, in bound or
 * not, or 2^64 - 1 when none does.  batch = 0: BA_OK, zero counters, witness
 * 2^64 - 1.  At most 2^40 strategies go into one launch.  Nothing is copied from
 * host memory: ba_smenum_run_device is fully asynchronous and may be captured in a
 * graph. */
#define BA_SMENUM_MESSAGES 0
#define BA_SMENUM_COALITION 1
/* B; host only.  0xFFFFFFFF for form > 1, n outside 1..32 or m > 8; saturates at
 * 0xFFFFFFFE. */
uint32_t ba_smenum_bits(uint32_t form, uint32_t n, uint32_t m, uint32_t faulty_mask);
/* bit i -> the message (round k[i], sender[i] -> recipient[i], value[i]); sender is
 * 0xFFFFFFFF ("any traitor") in the coalition form's relay rounds.  order decides
 * value[] only when the commander is loyal.  Host only.  Returns B, or BA_EINVAL (a
 * bad form / n / m / order, cap < B, a missing array). */
int ba_smenum_slots(uint32_t form, uint32_t n, uint32_t m, uint32_t faulty_mask, uint32_t order,
                    uint32_t* k, uint32_t* sender, uint32_t* recipient, uint32_t* value,
                    uint32_t cap);
int ba_smenum_run(struct ba_ctx* ctx, const ba_params* p, uint32_t form, uint32_t faulty_mask,
                  uint32_t order, uint64_t batch, uint64_t* decisions, uint8_t* outcome,
                  ba_counters* counters, uint64_t* witness);  /* counters and witness overwritten */
/* The same walk on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream).  d_counters is accumulated into; d_witness (optional)
 * is min-accumulated: the caller sets it to 2^64 - 1 first. */
int ba_smenum_run_device(struct ba_ctx* ctx, const ba_params* p, uint32_t form,
                         uint32_t faulty_mask, uint32_t order, uint64_t batch,
                         uint64_t* d_decisions, uint8_t* d_outcome, uint64_t* d_counters,
                         uint64_t* d_witness, void* stream);  /* accumulated, async */

/* ---- RAND against every traitor strategy and every coin outcome of one case ------
 * BA_KING_COIN and BA_KING_SPLIT do not see the coin; RAND's safety claim (no loyal
 * general ever decides two values or leaves a decided value) speaks of every choice
 * of messages and every fall of the coins.  These entries make both free bits and
 * walk all of them for one case (coin, n, m, R = phases, faulty set, order)
 * (docs/SEMANTICS.md §14; no ba.py analogue): each play of an adversary that sees
 * the coins is one (messages, coins) pair, so the walk covers it too.  The rules are
 * RAND's above, unchanged; every general, faulty ones included, keeps x, D and V and
 * runs the rules honestly.  Messages are truth / dead / free as in the King
 * enumeration: a dead report is retreat, a dead proposal is none; a free report or
 * round-0 send is one bit (1 = attack); a free proposal is two consecutive bits
 * (lo, hi), lo = 0 no proposal whatever hi is, lo = 1 proposes hi.  Tosses:
 *   BA_RAND_LOCAL   one free bit per loyal general and phase, read only where that
 *                   general has no v; a faulty general's own toss is dead (retreat);
 *   BA_RAND_COMMON  one free bit per phase, taken by every general that tosses.
 * With c = [0 in F], l = n - |F|, free bits ascend: round 0 (c l bits, by loyal
 * rank), then per phase the reports (sender's rank among the traitors * l + the
 * recipient's rank among the loyal), the proposals (twice that, lo then hi) and the
 * tosses (LOCAL: l bits by loyal rank; COMMON: one):
 *   B = c l + R (3 |F| l + (LOCAL ? l : 1))
 * The two "no proposal" codes and a toss bit nobody reads play alike, so rates are
 * rates over the coded space.  Trial t of a call is strategy S = t: a call covers S
 * in [p->first_trial, p->first_trial + batch), first_trial a multiple of 64, ending
 * at or below 2^B (else BA_EINVAL).  p supplies n, m and first_trial; seed and f are
 * unused.  p->lie_mode must be BA_LIE_PHILOX (TABLE: BA_ENOTSUP), p->engine
 * BA_ENGINE_AUTO, p->faulty_mode BA_FAULTY_GIVEN and p->order_mode BA_ORDER_GIVEN
 * (else BA_EINVAL); coin > 1, phases outside 1..BA_RENUM_MAX_PHASES, order >
 * BA_OTHER and m > 10 are BA_EINVAL.  B > BA_ENUM_MAX_BITS and n > 16 are
 * BA_ETOOBIG: the kernel keeps three planes per general in registers and is built
 * for n = 1..16.  One traitor alone costs at least 3 (n - 1) + 1 bits, over 48 from
 * n = 17 on, so what the n cap loses beyond the bit cap is only the cases without
 * any traitor (n in 17..32: B = R under COMMON, R n <= 48 under LOCAL).
 * decisions / outcome / counters / witness: as in the King enumeration, in-bound is
 * |F| <= m and n > 3m.  decided (optional, a byte per strategy): RAND's byte with its
 * precedence, BA_RAND_UNSAFE, the first phase p at whose end every loyal general has
 * D set (1 when nobody is loyal), BA_RAND_UNDECIDED.  stats (optional):
 *   stats[0] unsafe strategies (decided == 254)      stats[1] undecided (255)
 *   stats[2] smallest unsafe S    stats[3] smallest undecided S   (2^64-1: none)
 *   stats[3 + p], p = 1..16: strategies with decided == p
 *   stats[0] + stats[1] + sum_p stats[3 + p] == trials
 * batch = 0: BA_OK, zero counters and counts, the three witnesses 2^64 - 1.  At most
 * 2^40 strategies go into one launch.  Nothing is copied from host memory:
 * ba_renum_run_device is fully asynchronous and may be captured in a graph. */
#define BA_RENUM_MAX_PHASES 16
#define BA_RENUM_NSTATS 20
/* B; host only.  0xFFFFFFFF for coin > 1, n outside 1..32, m > 10 or phases outside
 * 1..16; saturates at 0xFFFFFFFE.  Not limited to n <= 16. */
uint32_t ba_renum_bits(uint32_t coin, uint32_t n, uint32_t m, uint32_t phases, uint32_t faulty_mask);
/* bit i -> the message (q[i], sender[i] -> recipient[i]) and part[i]: 0 for a one-bit
 * message, 0 / 1 for lo / hi of a proposal, 2 for a toss bit (q = 3p; sender =
 * recipient = the general under LOCAL, both 0xFFFFFFFF under COMMON); host only.
 * Returns B, or BA_EINVAL (bad arguments as above, cap < B, a missing array). */
int ba_renum_slots(uint32_t coin, uint32_t n, uint32_t m, uint32_t phases, uint32_t faulty_mask,
                   uint32_t* q, uint32_t* sender, uint32_t* recipient, uint32_t* part, uint32_t cap);
int ba_renum_run(struct ba_ctx* ctx, const ba_params* p, uint32_t coin, uint32_t phases,
                 uint32_t faulty_mask, uint32_t order, uint64_t batch, uint64_t* decisions,
                 uint8_t* outcome, uint8_t* decided, ba_counters* counters, uint64_t* witness,
                 uint64_t stats[BA_RENUM_NSTATS]);  /* counters, witness and stats overwritten */
/* The same walk on device buffers, enqueued on `stream` in the ctx's call order
 * (NULL = HIP's null stream).  d_counters and the counts of d_stats are accumulated
 * into; d_witness, d_stats[2] and d_stats[3] (d_witness and d_stats optional) are
 * min-accumulated: the caller sets them to 2^64 - 1 first. */
int ba_renum_run_device(struct ba_ctx* ctx, const ba_params* p, uint32_t coin, uint32_t phases,
                        uint32_t faulty_mask, uint32_t order, uint64_t batch,
                        uint64_t* d_decisions, uint8_t* d_outcome, uint8_t* d_decided,
                        uint64_t* d_counters, uint64_t* d_witness, uint64_t* d_stats,
                        void* stream);  /* accumulated, async */

/* ---- one huge instance split by first-hop subtree --------
 * The subtree of first-hop lieutenant j (relay paths starting 0 -> j) needs
 * only L_0[j]; its relay levels and inner majorities are independent of the
 * other subtrees.  A rank owning subtrees [j_begin, j_end) (0-based lieutenant
 * ranks, j_end <= n-1) computes their level-1 child results -- R_1[j.r]
 * (m_eff >= 2) or L_1[j.r] (m_eff == 1), the votes each lieutenant r counts
 * about j (ba.py:169-186 generalised) -- into
 *     d_votes[(j - j_begin)(n-2) + c][w],  w < ceil(batch/64), c < n-2,
 * 64 trials per uint64 word.  Concatenating every rank's d_votes in j order
 * (an all-gather) gives the full [(n-1)(n-2)][W] array that
 * ba_root_from_votes_device turns into the root majorities, quorum and
 * counters -- bit-identical to ba_run_trials_device on the same params.
 * Both are asynchronous on `stream` (NULL = HIP's null stream).
 * LEVELS engine, Philox lies; the batch must fit one scratch chunk
 * (BA_ETOOBIG otherwise: split the batch). */
uint64_t ba_vote_slots(uint32_t n, uint32_t m, uint32_t j_begin, uint32_t j_end);
int ba_subtree_votes_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                            uint32_t j_begin, uint32_t j_end, const uint32_t* d_faulty_mask,
                            const uint8_t* d_order, uint64_t* d_votes, void* stream);
int ba_root_from_votes_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                              const uint32_t* d_faulty_mask, const uint8_t* d_order,
                              const uint64_t* d_votes, uint64_t* d_decisions, uint8_t* d_outcome,
                              uint64_t* d_counters, void* stream);

/* ---- the same split at either of two levels ------------------------------
 * level 1 (BA_SPLIT_FIRST_HOP): units = the n-1 first-hop subtrees; exactly
 *   the entries above (votes R_1 / L_1, n-2 per unit).
 * level 2 (BA_SPLIT_SECOND_HOP): units = the (n-1)(n-2) second-hop subtrees,
 *   one per level-1 slot (j, a) in path order u = j(n-2) + k, a = k + (k >= j);
 *   a unit's relay levels >= 2 and majorities >= 2 need only L_1[j.a], so a
 *   rank owning units [u_begin, u_end) computes their level-2 results
 *   R_2[j.a.r] (n-3 per unit, receivers r in rank order) into
 *       d_votes[(u - u_begin)(n-3) + c][w].
 *   The root pass relays levels 0 and 1 itself (cheap: (n-1)^2 slots), takes
 *   the level-1 majorities over the gathered R_2 and finishes as above.  Needs
 *   m_eff >= 3.  15 first hops split 1,2,..,2 over 8 ranks (slowest rank 2/15
 *   of the tree); 210 second hops split 26/27 (27/210).
 * ba_split_units: the units of a level (0 if the level does not apply);
 * ba_split_vote_slots: vote rows of units [u_begin, u_end);
 * ba_split_share: rank's contiguous unit range, units split as evenly as
 * possible (ranks beyond the unit count get empty ranges).  The level-1 forms
 * equal ba_vote_slots / ba_subtree_share / ba_subtree_votes_device /
 * ba_root_from_votes_device. */
#define BA_SPLIT_FIRST_HOP 1
#define BA_SPLIT_SECOND_HOP 2
uint64_t ba_split_units(uint32_t n, uint32_t m, uint32_t level);
uint64_t ba_split_vote_slots(uint32_t n, uint32_t m, uint32_t level, uint32_t u_begin,
                             uint32_t u_end);
int ba_split_share(uint32_t n, uint32_t m, uint32_t level, int nranks, int rank,
                   uint32_t* u_begin, uint32_t* u_end);
int ba_split_votes_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch, uint32_t level,
                          uint32_t u_begin, uint32_t u_end, const uint32_t* d_faulty_mask,
                          const uint8_t* d_order, uint64_t* d_votes, void* stream);
int ba_root_from_split_votes_device(struct ba_ctx* ctx, const ba_params* p, uint64_t batch,
                                    uint32_t level, const uint32_t* d_faulty_mask,
                                    const uint8_t* d_order, const uint64_t* d_votes,
                                    uint64_t* d_decisions, uint8_t* d_outcome,
                                    uint64_t* d_counters, void* stream);

/* ---- multi-GPU (no ba.py analogue: its generals are threads of
 * one process, ba.py:104-112) ----------------------------------------------
 * One process per GPU.  Rank 0 calls ba_comm_unique_id and ships the
 * BA_COMM_ID_BYTES bytes to every rank out of band (MPI, a socket, a file, a
 * torch.distributed store); every rank calls ba_comm_create on its ctx (the
 * communicator owns an RCCL communicator, a counter buffer and a vote buffer,
 * and runs its whole jobs on the ctx's own stream; destroy a comm before its
 * ctx).  RCCL is opened at run time (librccl.so.1, or the copy already loaded
 * in the process).  Every rank of a comm must make the same sequence of
 * collective calls with the same params. */
#define BA_COMM_ID_BYTES 128
struct ba_comm;
int ba_ctx_device(struct ba_ctx* ctx, int* device);
/* The ctx's own non-blocking HIP stream (the one ba_run_trials uses), valid as
 * long as the ctx.  Callers without a HIP binding of their own (ctypes) can pass
 * it to the *_device entry points; ctxs created one after another get streams
 * on different hardware queues, so their calls can run concurrently. */
int ba_ctx_stream(struct ba_ctx* ctx, void** stream);
int ba_comm_unique_id(unsigned char id[BA_COMM_ID_BYTES]);
int ba_comm_create(struct ba_ctx* ctx, int nranks, int rank,
                   const unsigned char id[BA_COMM_ID_BYTES], struct ba_comm** out);
void ba_comm_destroy(struct ba_comm* comm);
int ba_comm_rank(struct ba_comm* comm, int* nranks, int* rank);
/* Watchdog of the blocking whole jobs below.  A job waits for its collectives
 * by polling the comm's stream; past `timeout_ms` (default 300000, or
 * BA_COMM_TIMEOUT_MS at ba_comm_create) it aborts the communicator
 * (ncclCommAbort: this rank's collectives return) and fails with BA_EABORTED.
 * That bounds every rank's wait when a peer left the protocol (a dead process,
 * or a rank whose own transport failed and which aborted itself: it cannot
 * tell its peers, RCCL has no such message, so they learn it from their own
 * watchdog).  ba_comm_abort does the same on demand (e.g. from a host-side
 * watchdog of the asynchronous collectives).  An aborted comm fails every
 * further call with BA_EABORTED; ba_comm_destroy still frees it. */
int ba_comm_set_timeout(struct ba_comm* comm, uint64_t timeout_ms);
int ba_comm_abort(struct ba_comm* comm);

/* Partition arithmetic (host only).  ba_trial_share: rank's contiguous,
 * 64-trial-word-aligned share [first, first + count) of total_trials, words
 * split as evenly as possible.  ba_subtree_share: rank's first-hop lieutenant
 * range [j_begin, j_end) of the n-1 subtrees (15 over 8 ranks: 1,2,2,2,2,2,2,2;
 * ranks beyond n-1 get empty ranges). */
int ba_trial_share(uint64_t total_trials, int nranks, int rank, uint64_t* first,
                   uint64_t* count);
int ba_subtree_share(uint32_t n, int nranks, int rank, uint32_t* j_begin, uint32_t* j_end);

/* Collectives, asynchronous on `stream` (a hipStream_t as void*).
 * ba_comm_allreduce_device: d_counters (BA_NCOUNTERS uint64) summed over the
 * ranks in place -- the only exchange trial-DP needs.
 * ba_comm_allgather_votes_device: d_votes is the full [(n-1)(n-2)][W] vote
 * array of ba_subtree_votes_device (W = ceil(batch/64)) in which every rank
 * has written the rows of its ba_subtree_share; afterwards every rank holds
 * every row (one grouped RCCL broadcast per rank: an all-gather of unequal
 * shares in place, no padding). */
int ba_comm_allreduce_device(struct ba_comm* comm, uint64_t* d_counters, void* stream);
int ba_comm_allgather_votes_device(struct ba_comm* comm, uint32_t n, uint32_t m, uint64_t batch,
                                   uint64_t* d_votes, void* stream);
/* the same all-gather for a split at `level` (d_votes: the full
 * [ba_split_vote_slots(n, m, level, 0, units)][W] array) */
int ba_comm_allgather_split_votes_device(struct ba_comm* comm, uint32_t n, uint32_t m,
                                         uint32_t level, uint64_t batch, uint64_t* d_votes,
                                         void* stream);

/* Whole jobs, blocking (they return after the collectives, on the comm's
 * stream).  A rank whose local work fails still joins every collective and
 * raises an error flag all-reduced with the counters: every rank then returns
 * an error, none blocks.
 * ba_run_trials_multi: trial-DP over [p->first_trial, + total_trials) --
 *   inputs drawn on the device (faulty/order modes other than GIVEN), Philox
 *   lies, every draw keyed by the global trial index; this rank's share of the
 *   decisions / outcome bytes goes to the optional device buffers
 *   (share_count entries); counters_out = the whole job's totals on every
 *   rank, equal to one unsharded ba_run_trials.
 * ba_run_instance_split_multi: `batch` (normally few, huge) instances split by
 *   first-hop subtree -- subtree votes, vote all-gather, root majorities and
 *   quorum; decisions / outcome (batch entries) and counters_out identical on
 *   every rank and equal to an unsplit ba_run_trials on the same params
 *   (Philox lies, given or drawn inputs).  With one rank the rank owns every
 *   subtree and the call is the unsplit pass itself. */
int ba_run_trials_multi(struct ba_ctx* ctx, struct ba_comm* comm, const ba_params* p,
                        uint64_t total_trials, uint64_t* d_decisions, uint8_t* d_outcome,
                        ba_counters* counters_out, uint64_t* share_first,
                        uint64_t* share_count);
int ba_run_instance_split_multi(struct ba_ctx* ctx, struct ba_comm* comm, const ba_params* p,
                                uint64_t batch, const uint32_t* d_faulty_mask,
                                const uint8_t* d_order, uint64_t* d_decisions,
                                uint8_t* d_outcome, ba_counters* counters_out);
/* ba_run_instance_split_multi at a split level (1 = the call above, 2 =
 * second-hop units, m_eff >= 3) */
int ba_run_instance_split_level_multi(struct ba_ctx* ctx, struct ba_comm* comm,
                                      const ba_params* p, uint32_t level, uint64_t batch,
                                      const uint32_t* d_faulty_mask, const uint8_t* d_order,
                                      uint64_t* d_decisions, uint8_t* d_outcome,
                                      ba_counters* counters_out);

/* Per-kernel timing (tracing aux subsystem; replaces nothing in ba.py, which
 * only prints).  When enabled, every kernel the ctx launches is bracketed by
 * HIP events on its launch stream; ba_profile_read syncs those events and
 * returns the index-th kernel's name, launch count and summed milliseconds
 * (BA_EINVAL past the last kernel).  Enabling/disabling clears the totals.
 * Launches on a stream that is capturing a graph are not bracketed: neither the
 * capture nor its replays add to the totals. */
int ba_profile_enable(struct ba_ctx* ctx, int on);
int ba_profile_read(struct ba_ctx* ctx, int index, char* name, int name_len,
                    uint64_t* launches, double* total_ms);

/* Engine-clock probe (measurement aux; no ba.py analogue).  Enqueues on `stream`
 * one tiny launch of BA_PROBE_BLOCKS one-wave blocks; block b writes
 * d_out[4b .. 4b+3] = {XCC id, HW id, s_memtime, s_memrealtime}.  s_memtime
 * counts shader-clock cycles on a PER-CU counter (counters of different CUs are
 * not aligned), s_memrealtime a constant 100 MHz clock, so two probes bracketing
 * a stretch of work give that stretch's average engine clock per XCD from rows
 * of the SAME CU (HW id bits 8-15): (dmemtime / drealtime) x 100 MHz
 * (MI355X_MICROARCH.md).  BA_PROBE_BLOCKS = 2048 one-wave blocks reach every CU
 * in each probe.  bench.py brackets a replica of its timed region with two. */
/* Device memory a ctx holds for the engines: the LEVELS scratch and the
 * cascade's fan-in counters, and the budget both are chunked to (environment
 * BA_SCRATCH_BYTES at ba_ctx_create, 8 GiB by default): scratch + counters <=
 * budget for every call the budget admits. */
int ba_ctx_memory(struct ba_ctx* ctx, uint64_t* scratch_bytes, uint64_t* counter_bytes,
                  uint64_t* budget_bytes);

#define BA_PROBE_BLOCKS 2048
int ba_clock_probe_device(struct ba_ctx* ctx, uint64_t* d_out, void* stream);

/* ---- ba.py's coin source (host only, no device needed) --------------------
 * Replaces the unseeded global CPython MT19937 behind random.randint(0, 1)
 * (ba.py:45 relay lies, ba.py:269 commander lies).  ba_mt_seed(s) equals
 * random.seed(s) for 0 <= s < 2^64; ba_mt_next32 equals random.getrandbits(32);
 * each coin is one random.randint(0, 1) draw (1 = "attack", i.e. the draw was
 * 0).  Coins are packed in BA_LIE_TABLE layout, in ba.py's canonical draw
 * order, so a table row feeds ba_run_trials directly. */
typedef struct ba_mt {
    uint32_t state[624];
    uint32_t index;
} ba_mt;

void ba_mt_seed(ba_mt* mt, uint64_t seed);
uint32_t ba_mt_next32(ba_mt* mt);
/* coins one ba.py round draws: (n-1) if the commander is faulty (ba.py:263-273),
 * plus, per lieutenant r, one per other faulty lieutenant and one for a faulty
 * commander it polls (ba.py:169-186).  m == 0: commander coins only. */
uint32_t ba_om1_coin_count(uint32_t n, uint32_t m, uint32_t faulty_mask, uint32_t poll_commander);
/* draw `count` coins into packed[0..words) (zeroed first) */
int ba_mt_draw_coins(ba_mt* mt, uint32_t count, uint32_t* packed, uint32_t words);
/* Batched replay table: trial t is random.seed(seeds[t]) followed by one ba.py
 * round over (faulty_mask[t], poll_commander[t] or 0); row t of `table`
 * (stride uint32 words) receives its coins; next_word[t] (optional) the next
 * getrandbits(32) after the round.  threads <= 0: all host cores. */
int ba_mt_table(uint32_t n, uint32_t m, uint64_t batch, const uint64_t* seeds,
                const uint32_t* faulty_mask, const uint32_t* poll_commander, uint32_t stride,
                uint32_t* table, uint32_t* next_word, int threads);
/* The same table on the device (device buffers, asynchronous on `stream`, in
 * the ctx's call order): one thread per trial seeds CPython's MT19937 and draws
 * the round's coins; the rows equal ba_mt_table's.  Feeds ba_run_trials_device
 * in BA_LIE_TABLE mode without a host round trip (tools/run_configs.py config 1).
 * Uses 2,496 B of the ctx's scratch per trial of a chunk. */
int ba_mt_table_device(struct ba_ctx* ctx, uint32_t n, uint32_t m, uint64_t batch,
                       const uint64_t* d_seeds, const uint32_t* d_faulty_mask,
                       const uint32_t* d_poll_commander, uint32_t stride, uint32_t* d_table,
                       uint32_t* d_next_word, void* stream);

/* Tree geometry helpers (host only, no device needed).  The slot counts are exact;
 * 0 for n outside 1..32 or m > 8 (ba_level_slots: and for k > min(m, n-2)). */
uint64_t ba_tree_slots(uint32_t n, uint32_t m);             /* sum_k |L_k|       */
uint64_t ba_level_slots(uint32_t n, uint32_t m, uint32_t k); /* |L_k|=P(n-1,k+1) */
int ba_engine_for(uint32_t n, uint32_t m);                  /* engine AUTO picks */

#ifdef __cplusplus
}
#endif
#endif
