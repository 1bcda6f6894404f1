"""Cases and the Python restatement for the batched Tick (etick_batch_device):
node.Tick() as tickElection / tickHeartbeat with promotable and
isElectionTimeout (raft/raft.go:287-307, 590-595, 608-617) over the records the
call reads.  raft.elapsed is Go's int: int64 that wraps, compared signed; the
rows hold its two's-complement bits.  Holds validate(), expected(), the
boundary lattice, the seeded random generators (random_scenario for the device,
draw_case / digest for tests/host/tick_forms.cpp, restated draw for draw), the
loader of the reference's table (tests/golden/raft_tick_kats.json) and
tickElection / tickHeartbeat over raft_model.Raft objects."""
import json
import os

import numpy as np

from vote_step_cases import SplitMix

M64 = (1 << 64) - 1
M63 = (1 << 63) - 1
OK, UNSUPPORTED = 0, 48
E_INVAL, E_NOMEM = -2, -3
IDLE, HELD, HUP, BEAT, NOT_PROMOTABLE, PANICKED = range(1, 7)
ACTION_NAMES = ("", "idle", "held", "hup", "beat", "not_promotable", "panicked")
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
GROUP_WORDS, VSTATE_WORDS, RESULT_WORDS, HUP_WORDS, BEAT_WORDS = 32, 8, 4, 8, 6
PEERS = 7
INT_MAX = (1 << 31) - 1
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_tick_kats.json")


# ---- the restatement -------------------------------------------------------------

def s64(x):
    """The uint64 bits x as Go's int."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def draw(seed, id, term, elapsed):
    """etick_draw, restated."""
    x = (seed ^ (id * 0x9E3779B97F4A7C15) ^ (term * 0xBF58476D1CE4E5B9) ^ (elapsed * 0x94D049BB133111EB)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 1


def tick(state, elapsed, id, term, n_peers, peer_id, election, heartbeat, r=None, seed=0):
    """One node.Tick(): (status, action, elapsed afterwards, draw consumed).  r
    is the rand.Int() value handed in; None: draw(seed, id, term, e)."""
    if n_peers > PEERS:
        return UNSUPPORTED, PANICKED, elapsed, 0
    if state == LEADER:                                   # tickHeartbeat
        e = (elapsed + 1) & M64
        if s64(e) > heartbeat:
            return OK, BEAT, 0, 0
        return OK, IDLE, e, 0
    if id not in list(peer_id)[:n_peers]:                 # tickElection: !promotable()
        return OK, NOT_PROMOTABLE, 0, 0
    e = (elapsed + 1) & M64
    d = s64(e - election)                                 # isElectionTimeout
    if d < 0:
        return OK, IDLE, e, 0
    if r is None:
        r = draw(seed, id, term, e)
    if d > r % election:
        return OK, HUP, 0, r
    return OK, HELD, e, r


# ---- a call ----------------------------------------------------------------------

def group(id=1, term=0, peers=(1,), n_peers=None, state=FOLLOWER, elapsed=0, draw=0, vote=0, lead=0):
    """One group of a call: what the tick reads, and the draw a d_draws array
    would hand it."""
    return dict(id=id, term=term, peers=tuple(peers), n_peers=len(peers) if n_peers is None else n_peers, state=state,
                elapsed=elapsed & M64, draw=draw, vote=vote, lead=lead)


def call_of(groups, election=10, heartbeat=1, sel=None, with_draws=False, seed=0, G=None, filler=None):
    """The arrays of one call.  groups[i] is selection i's group; with sel (a
    list of distinct group numbers, one per group) it lies at row sel[i] of G
    rows, the others hold `filler` rows (canaries: never looked at)."""
    n = len(groups)
    G = n if G is None else G
    grows = np.zeros((G, GROUP_WORDS), dtype=np.uint64)
    vrows = np.zeros((G, VSTATE_WORDS), dtype=np.uint64)
    if filler is not None:
        grows[:], vrows[:] = filler[0], filler[1]
    for i, g in enumerate(groups):
        at = i if sel is None else sel[i]
        row = [g["id"], g["term"], 0, 0, 0, 0, g["n_peers"]] + list(g["peers"][:PEERS])
        grows[at] = 0
        grows[at, :len(row)] = np.array(row, dtype=np.uint64)
        # match[] / next[] are not the tick's: any value must do
        grows[at, 14:28] = np.uint64(0x5555AAAA00000000 + i)
        vrows[at] = np.array([g["state"], g["vote"], g["lead"], g["elapsed"], 0, 0, 0, 0], dtype=np.uint64)
    return dict(groups=grows, vstate=vrows, G=G, n=n, sel=None if sel is None else [int(s) for s in sel],
                draws=[g["draw"] for g in groups] if with_draws else None, seed=seed, election=election,
                heartbeat=heartbeat)


def validate(a, hups_cap=None, beats_cap=None):
    """The whole-call status: E_INVAL, E_NOMEM or OK (caps None: the peek)."""
    if a["G"] >= INT_MAX or a["n"] >= INT_MAX:
        return E_INVAL
    if a["sel"] is None and a["n"] != a["G"]:
        return E_INVAL
    if (hups_cap is None) != (beats_cap is None):
        return E_INVAL
    if not 1 <= a["election"] <= INT_MAX or not 0 <= a["heartbeat"] <= INT_MAX:
        return E_INVAL
    seen = set()
    for i in range(a["n"]):
        g = i if a["sel"] is None else a["sel"][i]
        if g >= a["G"] or g in seen:
            return E_INVAL
        seen.add(g)
        gw, vw = [int(x) for x in a["groups"][g]], [int(x) for x in a["vstate"][g]]
        if vw[0] > 2 or any(gw[28:32]) or any(vw[6:8]):
            return E_INVAL
        slots = gw[7:7 + min(gw[6], PEERS)]
        if len(set(slots)) != len(slots):
            return E_INVAL
        if a["draws"] is not None and a["draws"][i] > M63:
            return E_INVAL
    if hups_cap is not None:
        x = expected(a)
        if x["n_hups"] > hups_cap or x["n_beats"] > beats_cap:
            return E_NOMEM
    return OK


def expected(a, emit=True):
    """What a valid call leaves: res_rows (n, 4), vstate (G, 8), hups (n_hups,
    8), beats (n_beats, 6), the counters and the outcomes as dicts.  emit False
    is the peek: vstate as it was, no rows."""
    vrows = a["vstate"].copy()
    res = np.zeros((a["n"], RESULT_WORDS), dtype=np.uint64)
    hups, beats, outcomes = [], [], []
    for i in range(a["n"]):
        g = i if a["sel"] is None else a["sel"][i]
        gw, vw = [int(x) for x in a["groups"][g]], [int(x) for x in a["vstate"][g]]
        r = None if a["draws"] is None else a["draws"][i]
        st, act, el, dr = tick(vw[0], vw[3], gw[0], gw[1], gw[6], gw[7:14], a["election"], a["heartbeat"], r, a["seed"])
        pos = 0
        if act == HUP:
            pos = len(hups)
            hups.append([g, 0, gw[0], 0, 0, 0, 0, 0])
        elif act == BEAT:
            pos = len(beats)
            beats.append([g, 1, 0, 0, 0, 0])
        res[i] = np.array([st | (act << 32), el, pos, dr], dtype=np.uint64)
        if emit:
            vrows[g, 3] = np.uint64(el)
        outcomes.append(dict(status=st, action=act, elapsed=el, out_pos=pos, draw=dr, group=g))
    return dict(res_rows=res, vstate=vrows,
                hups=np.array(hups, dtype=np.uint64).reshape(len(hups), HUP_WORDS) if emit else
                np.zeros((0, HUP_WORDS), np.uint64),
                beats=np.array(beats, dtype=np.uint64).reshape(len(beats), BEAT_WORDS) if emit else
                np.zeros((0, BEAT_WORDS), np.uint64),
                n_hups=len(hups), n_beats=len(beats), outcomes=outcomes)


def mix_of(outcomes):
    acts = [0] * 7
    for o in outcomes:
        acts[o["action"]] += 1
    return acts


# ---- the boundary lattice --------------------------------------------------------

ELECTIONS = (1, 2, 10, INT_MAX)


def lattice_groups(election, heartbeat):
    """Every boundary of the contract at one (election, heartbeat): elapsed x
    state x the peer list's shape x the draw."""
    el = {0, election - 2, election - 1, election, 2 * election - 2, 2 * election - 1, M63, M63 + 1, M64,
          heartbeat - 1, heartbeat, heartbeat + 1}
    peers7 = (11, 12, 13, 14, 15, 16, 17)
    shapes = [((), 0, 11), ((11,), 1, 11), ((11,), 1, 12),                     # n_peers 0; 1 promotable or not
              ((11, 12, 13), 3, 11), ((11, 12, 13), 3, 13), ((11, 12, 13), 3, 14),    # own id first, last, absent
              (peers7, 7, 11), (peers7, 7, 17), (peers7, 7, 18),
              ((11, 12, 13, 14), 3, 14),                                        # own id in a slot past n_peers
              (peers7, 8, 11)]                                                  # unsupported
    out = []
    for e in sorted(x & M64 for x in el):
        for state in (FOLLOWER, CANDIDATE, LEADER):
            for peers, np_, id_ in shapes:
                for dr in (0, election - 1, election, M63):
                    out.append(group(id=id_, term=len(out) % 5, peers=peers, n_peers=np_, state=state, elapsed=e,
                                     draw=dr, vote=len(out) % 3, lead=len(out) % 4))
    return out


def lattice_pairs():
    """The (election, heartbeat) pairs the lattice is built at."""
    return [(e, h) for e in ELECTIONS for h in (0, 1)] + [(10, 5), (10, INT_MAX)]


def permuted(n, G, seed):
    """n distinct group numbers of G, in a seeded order that is not sorted."""
    r = SplitMix(seed, n)
    idx = list(range(G))
    for k in range(G - 1, 0, -1):
        j = r.rnd(k + 1)
        idx[k], idx[j] = idx[j], idx[k]
    return idx[:n]


def canaries(G, seed):
    """Rows for groups no selection names: arbitrary words, invalid ones included."""
    r = SplitMix(seed, G)
    grows = np.array([[r.next() for _ in range(GROUP_WORDS)] for _ in range(G)], dtype=np.uint64)
    vrows = np.array([[r.next() for _ in range(VSTATE_WORDS)] for _ in range(G)], dtype=np.uint64)
    return grows, vrows


def lattice_calls(chunk=None):
    """The lattice crossed with d_sel NULL / permuted and d_draws given / NULL,
    as calls.  chunk: only that many groups of each lattice, from a seeded
    place (the small-n runs)."""
    calls = []
    for k, (election, heartbeat) in enumerate(lattice_pairs()):
        groups = lattice_groups(election, heartbeat)
        if chunk is not None:
            at = SplitMix(chunk, k).rnd(len(groups) - chunk + 1)
            groups = groups[at:at + chunk]
        for with_sel in (False, True):
            for with_draws in (False, True):
                n = len(groups)
                G = n + n // 2 + 3 if with_sel else n
                sel = permuted(n, G, 100 + k) if with_sel else None
                calls.append(call_of(groups, election, heartbeat, sel, with_draws, seed=0xC0FFEE + k, G=G,
                                     filler=canaries(G, k) if with_sel else None))
    return calls


# ---- the seeded generators -------------------------------------------------------

ELECTION_TABLE = (1, 2, 10, 10, 10, INT_MAX)
HEARTBEAT_TABLE = (0, 1, 1, 5)
STATE_TABLE = (FOLLOWER, FOLLOWER, FOLLOWER, CANDIDATE, LEADER, LEADER)
NP_TABLE = (0, 1, 3, 3, 3, 5, 7, 8)


def draw_case(seed, run):
    """One random tick, drawn exactly as tests/host/tick_forms.cpp draws it:
    (group, election, heartbeat, have_draw, r) -- r the draw itself, or the
    call's seed."""
    r = SplitMix(seed, run)
    election = ELECTION_TABLE[r.rnd(6)]
    heartbeat = HEARTBEAT_TABLE[r.rnd(4)]
    state = STATE_TABLE[r.rnd(6)]
    np_ = NP_TABLE[r.rnd(8)]
    peers = tuple(10 + 3 * k for k in range(PEERS))
    idmode, k = r.rnd(6), r.rnd(7)
    id_ = 999 if idmode == 0 else peers[0] if idmode == 1 else peers[k]
    term = r.rnd(5)
    emode, x, y = r.rnd(10), r.rnd(2), r.next()
    elapsed = (0, election - 2, election - 1, election, 2 * election - 2, 2 * election - 1, M63,
               (M63 + 1, M64)[x], election - 1 + y % election, heartbeat - 1 + y % 3)[emode] & M64
    have_draw, dmode, z = r.rnd(2), r.rnd(5), r.next()
    val = (0, election - 1, election, M63, z >> 1)[dmode] if have_draw else z
    g = group(id=id_, term=term, peers=peers, n_peers=np_, state=state, elapsed=elapsed, draw=val if have_draw else 0)
    return g, election, heartbeat, bool(have_draw), val


def fold(h, v):
    return ((h ^ (v & M64)) * 0x100000001B3) & M64


def digest(seed, runs):
    """(digest, the actions' counts, [ticks that took the shortcut, ticks that
    ran the modulo]) over draw_case(seed, 0 .. runs - 1), as tick_forms prints them."""
    h, acts, forms = 0xCBF29CE484222325, [0] * 7, [0, 0]
    for run in range(runs):
        g, election, heartbeat, have_draw, val = draw_case(seed, run)
        st, act, el, dr = tick(g["state"], g["elapsed"], g["id"], g["term"], g["n_peers"], g["peers"], election,
                               heartbeat, val if have_draw else None, val)
        acts[act] += 1
        if act in (HUP, HELD):
            d = s64(g["elapsed"] + 1 - election)
            forms[0 if d >= election else 1] += 1
        for v in (st, act, el, dr):
            h = fold(h, v)
    return h, acts, forms


def random_scenario(seed, n, with_sel=False, with_draws=False):
    """n random ticks as one call at election 10, heartbeat 1 (a call has one
    pair): draw_case's groups with their elapsed redrawn around these two."""
    groups = []
    for i in range(n):
        g, election, heartbeat, _, val = draw_case(seed, i)
        r = SplitMix(seed ^ 0x5EED, i)
        mode = r.rnd(8)
        g["elapsed"] = (0, 1, 8, 9, 9 + r.rnd(10), 9 + r.rnd(10), 18, M63)[mode]
        g["draw"] = val >> 1
        groups.append(g)
    G = 2 * n + 3 if with_sel else n
    sel = permuted(n, G, seed) if with_sel else None
    return call_of(groups, 10, 1, sel, with_draws, seed=seed * 0x9E3779B97F4A7C15 & M64, G=G,
                   filler=canaries(G, seed) if with_sel else None)


# ---- the reference's table -------------------------------------------------------

def load_kats():
    return json.load(open(KATS))


# ---- the model backend -----------------------------------------------------------

def tick_model(r, election, heartbeat, rand):
    """r.tick() on a raft_model.Raft: tickElection or tickHeartbeat without the
    Step at its end -- the message is returned ("hup" / "beat" / None) with the
    action, as the device hands it out, and the caller steps it.  rand(r, e) is
    rand.Int() for the node r at the incremented elapsed e."""
    if r.state == LEADER:
        return tickHeartbeat(r, heartbeat)
    return tickElection(r, election, rand)


def tickElection(r, election, rand):   # raft.go:288-298
    if not r.promotable():
        r.elapsed = 0
        return NOT_PROMOTABLE, None, 0
    r.elapsed = (r.elapsed + 1) & M64
    d = s64(r.elapsed - election)       # isElectionTimeout, raft.go:611-617
    if d < 0:
        return IDLE, None, 0
    v = rand(r, r.elapsed)
    if d > v % election:
        r.elapsed = 0
        return HUP, "hup", v
    return HELD, None, v


def tickHeartbeat(r, heartbeat):   # raft.go:301-307
    r.elapsed = (r.elapsed + 1) & M64
    if s64(r.elapsed) > heartbeat:
        r.elapsed = 0
        return BEAT, "beat", 0
    return IDLE, None, 0
