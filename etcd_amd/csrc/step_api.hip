// step_api.hip -- the host side of the batched raft step calls; included by
// ewal_api.hip inside its extern "C" region.  Every call is the same skeleton
// ("The step calls' common skeleton"): validate, carve the ctx's
// step scratch, count -> scan -> the one decision point -> apply.  The helpers
// below are that skeleton; an entry point keeps what is its own: its null and
// alignment lists, its scratch regions, its Args and its launches.

#define STEP_HEAD_SLOT 64           // bytes a head record's slot takes at the scratch's start
static_assert(sizeof(EleadHead) <= STEP_HEAD_SLOT && sizeof(ElogHead) <= STEP_HEAD_SLOT, "a head record's slot");

// the early-outs of every step call
static bool step_args_ok(const ewal_ctx *c, uint64_t n, uint64_t G) {
  return c && n < 0x7fffffffull && G < 0x7fffffffull;
}

// whether no pointer of the list has a bit of mask set (NULL passes)
static bool aligned(uintptr_t mask, std::initializer_list<const void *> ptrs) {
  uintptr_t bits = 0;
  for (const void *p : ptrs) bits |= (uintptr_t)p;
  return (bits & mask) == 0;
}

// the scratch's regions, in order: add() returns a region's offset
struct Carve {
  size_t end = 0;
  size_t add(size_t bytes, size_t align = 16) {
    const size_t off = (end + align - 1) & ~(align - 1);
    end = off + bytes;
    return off;
  }
  size_t size() const { return end; }
};

// Makes the device current, grows the step scratch to `need`, starts the
// call's timing and initialises its head words and the claim words at
// claim_off (0: the call claims no group).
static int step_begin(ewal_ctx *c, size_t need, size_t head_bytes, size_t claim_off, uint64_t G) {
  EW_CHECK(hipSetDevice(c->device));
  forget_records(c);
  EW_CHECK(c->lstep.ensure(need));
  uint8_t *base = c->lstep.as<uint8_t>();
  EW_CHECK(hipEventRecord(c->ev0, c->stream));
  EW_CHECK(hipMemsetAsync(base, 0, head_bytes, c->stream));
  if (claim_off && G) EW_CHECK(hipMemsetAsync(base + claim_off, 0xff, (size_t)G * 4, c->stream));
  return EWAL_OK;
}

// The one decision point: nothing of the caller's has been modified yet.  The
// call's n_heads (1 to 3) head records come back in h.
static int step_decide(ewal_ctx *c, const uint8_t *base, uint32_t n_heads, EleadHead *h) {
  EW_CHECK(hipGetLastError());
  uint8_t hb[3 * STEP_HEAD_SLOT];
  const size_t bytes = (size_t)(n_heads - 1) * STEP_HEAD_SLOT + sizeof(EleadHead);
  EW_CHECK(hipMemcpyAsync(hb, base, bytes, hipMemcpyDeviceToHost, c->stream));
  EW_CHECK(hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < n_heads; ++k) std::memcpy(&h[k], hb + k * STEP_HEAD_SLOT, sizeof(EleadHead));
  return EWAL_OK;
}

// the whole-call classes, then the capacity of the call's output (when it has one)
static int step_status(const EleadHead &h, bool have_out, uint64_t total, uint64_t cap) {
  if (h.errflag & STEP_ERR_INVAL) return EWAL_E_INVAL;
  if (h.errflag & STEP_ERR_NOMEM) return EWAL_E_NOMEM;
  if (have_out && total > cap) return EWAL_E_NOMEM;
  return EWAL_OK;
}

static int step_end(ewal_ctx *c) {
  EW_CHECK(hipGetLastError());
  EW_CHECK(hipEventRecord(c->ev1, c->stream));
  EW_CHECK(hipStreamSynchronize(c->stream));
  return EWAL_OK;
}

uint32_t elog_group_size(void) { return sizeof(elog_group); }
uint32_t elog_app_size(void) { return sizeof(elog_app); }
uint32_t elog_app_result_size(void) { return sizeof(elog_app_result); }
uint32_t elog_lane_max_entries(void) { return ELOG_LANE_MAX; }

static_assert(sizeof(elog_group) == 64 && sizeof(elog_app) == 64 && sizeof(elog_app_result) == 48 &&
                  sizeof(ewal_entry) == 40 && offsetof(emsg_out, reject) == 136,
              "elog_append layout");
int elog_append_batch_device(ewal_ctx *c, elog_group *d_groups, uint64_t G, uint64_t *d_terms, uint64_t n_terms,
                             const elog_app *d_apps, uint64_t n, const ewal_entry *d_ents, uint64_t n_ents_total,
                             elog_app_result *d_res, emsg_out *d_resp, uint64_t *n_accepted, uint64_t *n_appended) {
  if (n_accepted) *n_accepted = 0;
  if (n_appended) *n_appended = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_apps || !d_res || (n_terms && !d_terms) || (n_ents_total && !d_ents)) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_apps, d_res, d_resp}) || !aligned(7, {d_terms, d_ents})) return EWAL_E_INVAL;
  // scratch: head | claim[G] | wlist[n] | partial[2 * (lane workgroups + wave workgroups)]
  const uint32_t lane_blocks = grid_for(n, 256);
  const uint32_t wave_blocks_max =
      (uint32_t)std::min<uint64_t>(grid_for(n, 4), (uint64_t)std::max(1, c->num_cu) * 8);   // 32 waves a CU
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add((size_t)G * 4), o_wlist = cv.add((size_t)n * 4),
               o_part = cv.add(((size_t)lane_blocks + wave_blocks_max) * 16);
  if (int st = step_begin(c, cv.size(), sizeof(ElogHead), o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  ElogArgs a;
  a.groups = d_groups;
  a.G = G;
  a.terms = d_terms;
  a.n_terms = n_terms;
  a.apps = d_apps;
  a.n = n;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.res = d_res;
  a.resp = d_resp;
  a.head = (ElogHead *)base;
  a.claim = (uint32_t *)(base + o_claim);
  a.wlist = (uint32_t *)(base + o_wlist);
  a.partial = (unsigned long long *)(base + o_part);
  a.lane_blocks = lane_blocks;
  hipLaunchKernelGGL(k_lapp_check, dim3(lane_blocks), dim3(256), 0, c->stream, a);
  EW_CHECK(hipGetLastError());
  // the one decision point, on this call's own head record: the flag word and the work list's length
  ElogHead h;
  EW_CHECK(hipMemcpyAsync(&h, a.head, 8, hipMemcpyDeviceToHost, c->stream));
  EW_CHECK(hipStreamSynchronize(c->stream));
  if (h.errflag & STEP_ERR_INVAL) return EWAL_E_INVAL;
  if (h.errflag & STEP_ERR_NOMEM) return EWAL_E_NOMEM;
  const uint32_t wave_blocks = std::min<uint32_t>(grid_for(h.nlong, 4), wave_blocks_max);
  hipLaunchKernelGGL(k_lapp_lane, dim3(lane_blocks), dim3(256), 0, c->stream, a);
  if (wave_blocks) hipLaunchKernelGGL(k_lapp_wave, dim3(wave_blocks), dim3(256), 0, c->stream, a, h.nlong);
  hipLaunchKernelGGL(k_lapp_sum, dim3(1), dim3(256), 0, c->stream, (const unsigned long long *)a.partial,
                     lane_blocks + wave_blocks, a.head);
  // step_end with the totals' copy behind the end event, under the one sync
  EW_CHECK(hipGetLastError());
  EW_CHECK(hipEventRecord(c->ev1, c->stream));
  EW_CHECK(hipMemcpyAsync(&h, a.head, sizeof(ElogHead), hipMemcpyDeviceToHost, c->stream));
  EW_CHECK(hipStreamSynchronize(c->stream));
  if (n_accepted) *n_accepted = h.accepted;
  if (n_appended) *n_appended = h.appended;
  return EWAL_OK;
}

uint32_t elead_group_size(void) { return sizeof(elead_group); }
uint32_t elead_snap_size(void) { return sizeof(elead_snap); }
uint32_t elead_resp_size(void) { return sizeof(elead_resp); }
uint32_t elead_result_size(void) { return sizeof(elead_result); }

static_assert(sizeof(elead_group) == 256 && sizeof(elead_snap) == 64 && sizeof(elead_resp) == 48 &&
                  sizeof(elead_result) == 48 && offsetof(elead_group, match) == 112 &&
                  offsetof(elead_group, reserved) == 224 && offsetof(emsg_out, snap_index) == 72,
              "elead_step layout");
int elead_step_batch_device(ewal_ctx *c, elead_group *d_groups, uint64_t G, const elead_snap *d_snaps,
                            const ewal_entry *d_ents, uint64_t n_ents_total, const elead_resp *d_resps, uint64_t n,
                            elead_result *d_res, emsg_out *d_msgs, uint64_t msgs_cap, uint64_t *n_msgs,
                            uint64_t *n_committed) {
  if (n_msgs) *n_msgs = 0;
  if (n_committed) *n_committed = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_resps || !d_res || (n_ents_total && !d_ents)) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_snaps, d_resps, d_res, d_msgs}) || !aligned(7, {d_ents})) return EWAL_E_INVAL;
  // scratch: head | claim[G] | run_msgs[n] | partial[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add((size_t)G * 4), o_run = cv.add((size_t)n * 8), o_part = cv.add((size_t)blocks * 16, 8);
  if (int st = step_begin(c, cv.size(), sizeof(EleadHead), o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EleadArgs a;
  a.groups = d_groups;
  a.G = G;
  a.snaps = d_snaps;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.resps = d_resps;
  a.n = n;
  a.res = d_res;
  a.msgs = d_msgs;
  a.head = (EleadHead *)base;
  a.claim = (uint32_t *)(base + o_claim);
  a.run_msgs = (unsigned long long *)(base + o_run);
  a.partial = (unsigned long long *)(base + o_part);
  hipLaunchKernelGGL(k_lead_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.partial, blocks, a.head);
  EleadHead h;
  if (int st = step_decide(c, base, 1, &h)) return st;
  if (int st = step_status(h, d_msgs, h.n_msgs, msgs_cap)) return st;
  if (d_msgs)
    hipLaunchKernelGGL(k_lead_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_lead_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_msgs) *n_msgs = h.n_msgs;
  if (n_committed) *n_committed = h.n_committed;
  return EWAL_OK;
}

uint32_t elead_prop_state_size(void) { return sizeof(elead_prop_state); }
uint32_t elead_local_size(void) { return sizeof(elead_local); }
uint32_t elead_local_result_size(void) { return sizeof(elead_local_result); }

static_assert(sizeof(elead_prop_state) == 32 && sizeof(elead_local) == 48 && sizeof(elead_local_result) == 48 &&
                  offsetof(elead_local, data_off) == 24 && offsetof(elead_local_result, index) == 24 &&
                  offsetof(elead_group, nlog) == 32,
              "elead_local layout");
int elead_local_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_state, uint64_t G,
                             const elead_snap *d_snaps, ewal_entry *d_ents, uint64_t n_ents_total,
                             uint64_t data_len_total, const elead_local *d_locals, uint64_t n,
                             elead_local_result *d_res, emsg_out *d_msgs, uint64_t msgs_cap, uint64_t *n_msgs,
                             uint64_t *n_appended) {
  if (n_msgs) *n_msgs = 0;
  if (n_appended) *n_appended = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_state || !d_locals || !d_res || (n_ents_total && !d_ents)) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_state, d_snaps, d_locals, d_res, d_msgs}) || !aligned(7, {d_ents}))
    return EWAL_E_INVAL;
  // scratch: head | claim[G] | seg[n] | cnt[n] | agg[workgroups] | partial[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add((size_t)G * 4), o_seg = cv.add((size_t)n * 8), o_cnt = cv.add((size_t)n * 8, 8),
               o_agg = cv.add((size_t)blocks * 16), o_part = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), sizeof(EleadHead), o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EpropArgs a;
  a.groups = d_groups;
  a.state = d_state;
  a.G = G;
  a.snaps = d_snaps;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.data_len_total = data_len_total;
  a.locals = d_locals;
  a.n = n;
  a.res = d_res;
  a.msgs = d_msgs;
  a.head = (EleadHead *)base;
  a.claim = (uint32_t *)(base + o_claim);
  a.seg = (unsigned long long *)(base + o_seg);
  a.cnt = (unsigned long long *)(base + o_cnt);
  a.agg = (EpropAgg *)(base + o_agg);
  a.partial = (unsigned long long *)(base + o_part);
  hipLaunchKernelGGL(k_prop_check, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_prop_carry, dim3(1), dim3(256), 0, c->stream, a.agg, blocks);
  hipLaunchKernelGGL(k_prop_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.partial, blocks, a.head);
  EleadHead h;
  if (int st = step_decide(c, base, 1, &h)) return st;
  if (int st = step_status(h, d_msgs, h.n_msgs, msgs_cap)) return st;
  if (d_msgs) {
    hipLaunchKernelGGL(k_prop_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_prop_commit, dim3(blocks), dim3(256), 0, c->stream, a);
  } else {
    hipLaunchKernelGGL(k_prop_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  }
  if (int st = step_end(c)) return st;
  if (n_msgs) *n_msgs = h.n_msgs;
  if (n_appended) *n_appended = h.n_committed;
  return EWAL_OK;
}

uint32_t evote_state_size(void) { return sizeof(evote_state); }
uint32_t evote_msg_size(void) { return sizeof(evote_msg); }
uint32_t evote_result_size(void) { return sizeof(evote_result); }

static_assert(sizeof(evote_state) == 64 && sizeof(evote_msg) == 64 && sizeof(evote_result) == 48 &&
                  offsetof(evote_state, voted) == 32 && offsetof(evote_msg, reject) == 48 &&
                  offsetof(evote_result, term) == 24 && offsetof(evote_result, state) == 40,
              "evote_step layout");
int evote_step_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                            uint64_t G, const elead_snap *d_snaps, ewal_entry *d_ents, uint64_t n_ents_total,
                            const evote_msg *d_in, uint64_t n, evote_result *d_res, emsg_out *d_msgs,
                            uint64_t msgs_cap, uint64_t *n_msgs, uint64_t *n_won) {
  if (n_msgs) *n_msgs = 0;
  if (n_won) *n_won = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_vstate || !d_in || !d_res || (n_ents_total && !d_ents)) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_vstate, d_snaps, d_in, d_res, d_msgs}) || !aligned(7, {d_ents}))
    return EWAL_E_INVAL;
  // scratch: head | claim[G] | fterm[n] | run_msgs[n] | partial[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add((size_t)G * 4), o_ft = cv.add((size_t)n * 8), o_run = cv.add((size_t)n * 8, 8),
               o_part = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), sizeof(EleadHead), o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EvoteArgs a{};
  a.p.groups = d_groups;
  a.p.state = d_pstate;
  a.p.G = G;
  a.p.snaps = d_snaps;
  a.p.ents = d_ents;
  a.p.n_ents_total = n_ents_total;
  a.p.n = n;
  a.p.msgs = d_msgs;
  a.p.head = (EleadHead *)base;
  a.p.claim = (uint32_t *)(base + o_claim);
  a.p.partial = (unsigned long long *)(base + o_part);
  a.vstate = d_vstate;
  a.in = d_in;
  a.n = n;
  a.res = d_res;
  a.fterm = (unsigned long long *)(base + o_ft);
  a.run_msgs = (unsigned long long *)(base + o_run);
  hipLaunchKernelGGL(k_vote_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.p.partial, blocks, a.p.head);
  EleadHead h;
  if (int st = step_decide(c, base, 1, &h)) return st;
  if (int st = step_status(h, d_msgs, h.n_msgs, msgs_cap)) return st;
  if (d_msgs)
    hipLaunchKernelGGL(k_vote_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_vote_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_msgs) *n_msgs = h.n_msgs;
  if (n_won) *n_won = h.n_committed;
  return EWAL_OK;
}

uint32_t eready_state_size(void) { return sizeof(eready_state); }
uint32_t eready_result_size(void) { return sizeof(eready_result); }

static_assert(sizeof(eready_state) == 64 && sizeof(eready_result) == 96 && sizeof(ewal_save_rec) == 56 &&
                  sizeof(ewal_entry) == 40 && sizeof(EreadyRec) == 32 && offsetof(eready_state, applied) == 48 &&
                  offsetof(eready_result, ents_first) == 32 && offsetof(eready_result, save_first) == 64 &&
                  offsetof(eready_result, state) == 88 && offsetof(ewal_save_rec, data_nil) == 48,
              "eready layout");
int eready_batch_device(ewal_ctx *c, const elead_group *d_groups, elead_prop_state *d_pstate,
                        const evote_state *d_vstate, eready_state *d_rstate, uint64_t G, const elead_snap *d_snaps,
                        const ewal_entry *d_ents, uint64_t n_ents_total, const uint64_t *d_sel, uint64_t n,
                        eready_result *d_res, ewal_save_rec *d_save, uint64_t save_cap, uint64_t *n_save,
                        uint64_t *n_ready) {
  if (n_save) *n_save = 0;
  if (n_ready) *n_ready = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (!d_sel && n != G) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_vstate || !d_rstate || !d_res || (n_ents_total && !d_ents)) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_vstate, d_rstate, d_snaps, d_res, d_save}) || !aligned(7, {d_ents, d_sel}))
    return EWAL_E_INVAL;
  // scratch: head | claim[G] (with d_sel: without it no group can be named twice) | rec[n] | partial[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add(d_sel ? (size_t)G * 4 : 0), o_rec = cv.add((size_t)n * sizeof(EreadyRec)),
               o_part = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), sizeof(EleadHead), d_sel ? o_claim : 0, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EreadyArgs a{};
  a.groups = d_groups;
  a.pstate = d_pstate;
  a.vstate = d_vstate;
  a.rstate = d_rstate;
  a.G = G;
  a.snaps = d_snaps;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.sel = d_sel;
  a.n = n;
  a.res = d_res;
  a.save = d_save;
  a.blocks = blocks;
  a.head = (EleadHead *)base;
  a.claim = (uint32_t *)(base + o_claim);
  a.rec = (EreadyRec *)(base + o_rec);
  a.partial = (unsigned long long *)(base + o_part);
  hipLaunchKernelGGL(k_ready_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.partial, blocks, a.head);
  EleadHead h;
  if (int st = step_decide(c, base, 1, &h)) return st;
  if (int st = step_status(h, d_save, h.n_msgs, save_cap)) return st;
  a.n_save = h.n_msgs;
  if (d_save)
    hipLaunchKernelGGL(k_ready_emit<true>, dim3(std::max(blocks, grid_for(a.n_save, 256))), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_ready_emit<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_save) *n_save = h.n_msgs;
  if (n_ready) *n_ready = h.n_committed;
  return EWAL_OK;
}

uint32_t efollow_msg_size(void) { return sizeof(efollow_msg); }
uint32_t efollow_result_size(void) { return sizeof(efollow_result); }

static_assert(sizeof(efollow_msg) == 96 && sizeof(efollow_result) == 96 && sizeof(EfollowCopy) == 48 &&
                  offsetof(efollow_msg, ents_first) == 56 && offsetof(efollow_msg, snap) == 80 &&
                  offsetof(efollow_result, conflict) == 24 && offsetof(efollow_result, dst_first) == 48 &&
                  offsetof(efollow_result, state) == 80 && offsetof(eready_state, applied) == 48 &&
                  offsetof(elead_snap, nodes_off) == 32,
              "efollow layout");
int efollow_step_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                              eready_state *d_rstate, uint64_t G, elead_snap *d_snaps, ewal_entry *d_ents,
                              uint64_t n_ents_total, const ewal_entry *d_src, uint64_t n_src_total,
                              const elead_snap *d_in_snaps, uint64_t n_in_snaps, const uint64_t *d_u64, uint64_t n_u64,
                              const efollow_msg *d_in, uint64_t n, efollow_result *d_res, emsg_out *d_msgs,
                              uint64_t msgs_cap, uint64_t *n_msgs, uint64_t *n_appended, uint64_t *n_restored) {
  if (n_msgs) *n_msgs = 0;
  if (n_appended) *n_appended = 0;
  if (n_restored) *n_restored = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_vstate || !d_in || !d_res || (n_ents_total && !d_ents) || (n_src_total && !d_src) ||
      (n_in_snaps && !d_in_snaps) || (n_u64 && !d_u64))
    return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_vstate, d_rstate, d_snaps, d_in_snaps, d_in, d_res, d_msgs}) ||
      !aligned(7, {d_ents, d_src, d_u64}))
    return EWAL_E_INVAL;
  // scratch: head | copy head | claim[G] | run_msgs[n] | cp[n] | partial[2 * workgroups] | cpart[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_chead = cv.add(STEP_HEAD_SLOT), o_claim = cv.add((size_t)G * 4), o_run = cv.add((size_t)n * 8),
               o_cp = cv.add((size_t)n * sizeof(EfollowCopy)), o_part = cv.add((size_t)blocks * 16),
               o_cpart = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), 2 * STEP_HEAD_SLOT, o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EfollowArgs a{};
  a.p.groups = d_groups;
  a.p.state = d_pstate;
  a.p.G = G;
  a.p.snaps = d_snaps;
  a.p.ents = d_ents;
  a.p.n_ents_total = n_ents_total;
  a.p.n = n;
  a.p.msgs = d_msgs;
  a.p.head = (EleadHead *)base;
  a.p.claim = (uint32_t *)(base + o_claim);
  a.p.partial = (unsigned long long *)(base + o_part);
  a.vstate = d_vstate;
  a.rstate = d_rstate;
  a.snaps = d_snaps;
  a.src = d_src;
  a.n_src_total = n_src_total;
  a.in_snaps = d_in_snaps;
  a.n_in_snaps = n_in_snaps;
  a.u64 = d_u64;
  a.n_u64 = n_u64;
  a.in = d_in;
  a.n = n;
  a.res = d_res;
  a.run_msgs = (unsigned long long *)(base + o_run);
  a.cp = (EfollowCopy *)(base + o_cp);
  a.cpart = (unsigned long long *)(base + o_cpart);
  a.chead = (EleadHead *)(base + o_chead);
  a.blocks = blocks;
  hipLaunchKernelGGL(k_follow_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.p.partial, blocks, a.p.head);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.cpart, blocks, a.chead);
  EleadHead h[2];                                    // the messages and RESTORED records; the copied entries
  if (int st = step_decide(c, base, 2, h)) return st;
  if (int st = step_status(h[0], d_msgs, h[0].n_msgs, msgs_cap)) return st;
  a.n_copy = h[1].n_msgs;
  if (d_msgs) {
    hipLaunchKernelGGL(k_follow_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
    if (a.n_copy) hipLaunchKernelGGL(k_follow_copy, dim3(grid_for(a.n_copy, 256)), dim3(256), 0, c->stream, a);
  } else {
    hipLaunchKernelGGL(k_follow_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  }
  if (int st = step_end(c)) return st;
  if (n_msgs) *n_msgs = h[0].n_msgs;
  if (n_appended) *n_appended = h[1].n_msgs;
  if (n_restored) *n_restored = h[0].n_committed;
  return EWAL_OK;
}

uint32_t ecompact_req_size(void) { return sizeof(ecompact_req); }
uint32_t ecompact_result_size(void) { return sizeof(ecompact_result); }

static_assert(sizeof(ecompact_req) == 96 && sizeof(ecompact_result) == 64 && sizeof(EcompactMove) == 48 &&
                  offsetof(ecompact_req, data_off) == 32 && offsetof(ecompact_req, removed_off) == 64 &&
                  offsetof(ecompact_result, n_left) == 24 && offsetof(ecompact_result, unstable) == 56 &&
                  offsetof(eready_state, applied) == 48 && offsetof(elead_group, log_offset) == 24 &&
                  offsetof(elead_prop_state, unstable) == 8,
              "ecompact layout");
int ecompact_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_pstate, const eready_state *d_rstate,
                          uint64_t G, elead_snap *d_snaps, ewal_entry *d_ents, uint64_t n_ents_total,
                          uint64_t data_len_total, uint64_t n_u64, const ecompact_req *d_reqs, uint64_t n,
                          ecompact_result *d_res, uint32_t flags, uint64_t *n_compacted, uint64_t *n_moved) {
  if (n_compacted) *n_compacted = 0;
  if (n_moved) *n_moved = 0;
  if (!step_args_ok(c, n, G) || (flags & ~(uint32_t)ECOMPACT_PEEK) != 0) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_rstate || !d_snaps || !d_reqs || !d_res || (n_ents_total && !d_ents))
    return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_rstate, d_snaps, d_reqs, d_res}) || !aligned(7, {d_ents}))
    return EWAL_E_INVAL;
  // scratch: head | overlap head | claim[G] | mv[n] | dpart[2 * workgroups] | opart[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_ohead = cv.add(STEP_HEAD_SLOT), o_claim = cv.add((size_t)G * 4),
               o_mv = cv.add((size_t)n * sizeof(EcompactMove)), o_dpart = cv.add((size_t)blocks * 16),
               o_opart = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), 2 * STEP_HEAD_SLOT, o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EcompactArgs a{};
  a.p.groups = d_groups;
  a.p.state = d_pstate;
  a.p.G = G;
  a.p.ents = d_ents;
  a.p.n_ents_total = n_ents_total;
  a.p.data_len_total = data_len_total;
  a.p.n = n;
  a.p.head = (EleadHead *)base;
  a.p.claim = (uint32_t *)(base + o_claim);
  a.rstate = d_rstate;
  a.snaps = d_snaps;
  a.n_u64 = n_u64;
  a.in = d_reqs;
  a.n = n;
  a.res = d_res;
  a.mv = (EcompactMove *)(base + o_mv);
  a.dpart = (unsigned long long *)(base + o_dpart);
  a.opart = (unsigned long long *)(base + o_opart);
  a.ohead = (EleadHead *)(base + o_ohead);
  a.blocks = blocks;
  hipLaunchKernelGGL(k_compact_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.dpart, blocks, a.p.head);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.opart, blocks, a.ohead);
  EleadHead h[2];                                    // the disjoint entries and COMPACTED requests; the overlapping entries
  if (int st = step_decide(c, base, 2, h)) return st;
  if (int st = step_status(h[0], false, 0, 0)) return st;
  const uint64_t n_dis = h[0].n_msgs, n_ov = h[1].n_msgs;
  if (flags & ECOMPACT_PEEK) {
    hipLaunchKernelGGL(k_compact_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  } else {
    if (n_ov) {
      EW_CHECK(c->lcompact_stage.ensure((size_t)n_ov * sizeof(ewal_entry)));
      a.stage = c->lcompact_stage.as<ewal_entry>();
    }
    // the apply pass reads the snapshot's term where the call found it: before any move
    hipLaunchKernelGGL(k_compact_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
    if (n_dis) {
      a.n_move = n_dis;
      hipLaunchKernelGGL(k_compact_move<MV_DIRECT>, dim3(grid_for(n_dis, 256)), dim3(256), 0, c->stream, a);
    }
    if (n_ov) {
      a.n_move = n_ov;
      hipLaunchKernelGGL(k_compact_move<MV_GATHER>, dim3(grid_for(n_ov, 256)), dim3(256), 0, c->stream, a);
      hipLaunchKernelGGL(k_compact_move<MV_SCATTER>, dim3(grid_for(n_ov, 256)), dim3(256), 0, c->stream, a);
    }
  }
  if (int st = step_end(c)) return st;
  if (n_compacted) *n_compacted = h[0].n_committed;
  if (n_moved) *n_moved = n_dis + n_ov;
  return EWAL_OK;
}

uint32_t etick_result_size(void) { return sizeof(etick_result); }
uint64_t etick_draw(uint64_t seed, uint64_t id, uint64_t term, uint64_t elapsed) {
  return tick_step::draw(seed, id, term, elapsed);
}

static_assert(sizeof(etick_result) == 32 && sizeof(EtickRec) == 32 && offsetof(etick_result, elapsed) == 8 &&
                  offsetof(etick_result, draw) == 24 && offsetof(elead_group, match) == 112 &&
                  offsetof(elead_group, n_peers) == 48 && offsetof(evote_state, elapsed) == 24 &&
                  offsetof(evote_msg, from) == 16 && sizeof(elead_local) == 48,
              "etick layout");
int etick_batch_device(ewal_ctx *c, const elead_group *d_groups, evote_state *d_vstate, uint64_t G,
                       const uint64_t *d_sel, uint64_t n, int64_t election, int64_t heartbeat, const uint64_t *d_draws,
                       uint64_t seed, etick_result *d_res, evote_msg *d_hups, uint64_t hups_cap, elead_local *d_beats,
                       uint64_t beats_cap, uint64_t *n_hups, uint64_t *n_beats) {
  if (n_hups) *n_hups = 0;
  if (n_beats) *n_beats = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (!d_sel && n != G) return EWAL_E_INVAL;
  if ((d_hups == nullptr) != (d_beats == nullptr)) return EWAL_E_INVAL;
  if (election < 1 || election > 0x7fffffffll || heartbeat < 0 || heartbeat > 0x7fffffffll) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_vstate || !d_res) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_vstate, d_res, d_hups, d_beats}) || !aligned(7, {d_sel, d_draws})) return EWAL_E_INVAL;
  // scratch: head | msgBeat head | claim[G] (with d_sel) | rec[n] | hpart[2 * workgroups] | bpart[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_bhead = cv.add(STEP_HEAD_SLOT), o_claim = cv.add(d_sel ? (size_t)G * 4 : 0),
               o_rec = cv.add((size_t)n * sizeof(EtickRec)), o_hpart = cv.add((size_t)blocks * 16),
               o_bpart = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), 2 * STEP_HEAD_SLOT, d_sel ? o_claim : 0, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EtickArgs a{};
  a.groups = d_groups;
  a.vstate = d_vstate;
  a.G = G;
  a.sel = d_sel;
  a.n = n;
  a.election = election;
  a.heartbeat = heartbeat;
  a.draws = d_draws;
  a.seed = seed;
  a.res = d_res;
  a.hups = d_hups;
  a.beats = d_beats;
  a.claim = (uint32_t *)(base + o_claim);
  a.rec = (EtickRec *)(base + o_rec);
  a.hpart = (unsigned long long *)(base + o_hpart);
  a.bpart = (unsigned long long *)(base + o_bpart);
  a.head = (EleadHead *)base;
  a.bhead = (EleadHead *)(base + o_bhead);
  hipLaunchKernelGGL(k_tick_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.hpart, blocks, a.head);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.bpart, blocks, a.bhead);
  EleadHead h;                                       // n_msgs: the msgHup, n_committed: the msgBeat
  if (int st = step_decide(c, base, 1, &h)) return st;
  const bool emit = d_hups != nullptr;
  if (int st = step_status(h, emit, h.n_msgs, hups_cap)) return st;
  if (int st = step_status(h, emit, h.n_committed, beats_cap)) return st;
  if (emit)
    hipLaunchKernelGGL(k_tick_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_tick_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_hups) *n_hups = h.n_msgs;
  if (n_beats) *n_beats = h.n_committed;
  return EWAL_OK;
}

uint32_t econf_state_size(void) { return sizeof(econf_state); }
uint32_t econf_req_size(void) { return sizeof(econf_req); }
uint32_t econf_result_size(void) { return sizeof(econf_result); }
uint32_t econf_applied_size(void) { return sizeof(econf_applied); }
uint32_t econf_scan_result_size(void) { return sizeof(econf_scan_result); }
uint32_t econf_gate_result_size(void) { return sizeof(econf_gate_result); }

static_assert(sizeof(econf_state) == 128 && sizeof(econf_req) == 32 && sizeof(econf_result) == 48 &&
                  sizeof(econf_applied) == 32 && sizeof(econf_scan_result) == 48 && sizeof(econf_gate_result) == 32 &&
                  sizeof(EcscanRec) == 48 && sizeof(EgateRec) == 32 && offsetof(econf_state, reserved) == 120 &&
                  offsetof(econf_result, n_peers) == 24 && offsetof(econf_scan_result, bad_pos) == 24 &&
                  offsetof(eready_result, committed_first) == 48 && offsetof(eready_state, soft_dirty) == 56 &&
                  offsetof(elead_snap, removed_off) == 48 && offsetof(elead_prop_state, pending_conf) == 16 &&
                  sizeof(emsg_out) == 144,
              "econf layout");
int econf_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                       eready_state *d_rstate, econf_state *d_cstate, uint64_t G, const elead_snap *d_snaps,
                       const uint64_t *d_u64, uint64_t n_u64, const econf_req *d_reqs, uint64_t n, econf_result *d_res,
                       emsg_out *d_msgs, uint64_t msgs_cap, uint64_t *n_msgs, uint64_t *n_changed) {
  if (n_msgs) *n_msgs = 0;
  if (n_changed) *n_changed = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_vstate || !d_rstate || !d_cstate || !d_reqs || !d_res || (n_u64 && !d_u64))
    return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_vstate, d_rstate, d_cstate, d_snaps, d_reqs, d_res, d_msgs}) ||
      !aligned(7, {d_u64}))
    return EWAL_E_INVAL;
  // scratch: head | claim[G] | run_msgs[n] | partial[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_claim = cv.add((size_t)G * 4), o_run = cv.add((size_t)n * 8), o_part = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), sizeof(EleadHead), o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EconfArgs a{};
  a.groups = d_groups;
  a.pstate = d_pstate;
  a.vstate = d_vstate;
  a.rstate = d_rstate;
  a.cstate = d_cstate;
  a.G = G;
  a.snaps = d_snaps;
  a.u64 = d_u64;
  a.n_u64 = n_u64;
  a.in = d_reqs;
  a.n = n;
  a.res = d_res;
  a.msgs = d_msgs;
  a.head = (EleadHead *)base;
  a.claim = (uint32_t *)(base + o_claim);
  a.run_msgs = (unsigned long long *)(base + o_run);
  a.partial = (unsigned long long *)(base + o_part);
  hipLaunchKernelGGL(k_conf_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.partial, blocks, a.head);
  EleadHead h;
  if (int st = step_decide(c, base, 1, &h)) return st;
  if (int st = step_status(h, d_msgs, h.n_msgs, msgs_cap)) return st;
  if (d_msgs)
    hipLaunchKernelGGL(k_conf_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_conf_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_msgs) *n_msgs = h.n_msgs;
  if (n_changed) *n_changed = h.n_committed;
  return EWAL_OK;
}

int econf_scan_committed_device(ewal_ctx *c, const eready_result *d_ready, const uint64_t *d_sel, uint64_t n,
                                uint64_t G, const ewal_entry *d_ents, uint64_t n_ents_total, const void *d_data,
                                uint64_t data_len_total, econf_scan_result *d_scan, econf_req *d_reqs,
                                econf_applied *d_applied, uint64_t reqs_cap, uint64_t *n_reqs, uint64_t *n_entries) {
  if (n_reqs) *n_reqs = 0;
  if (n_entries) *n_entries = 0;
  if (!step_args_ok(c, n, G) || n_ents_total >= 0x7fffffffull) return EWAL_E_INVAL;
  if (!d_sel && n != G) return EWAL_E_INVAL;
  if ((d_reqs == nullptr) != (d_applied == nullptr)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_ready || !d_scan || (n_ents_total && !d_ents) || (data_len_total && !d_data)) return EWAL_E_INVAL;
  if (!aligned(15, {d_ready, d_scan, d_reqs, d_applied}) || !aligned(7, {d_ents, d_sel})) return EWAL_E_INVAL;
  // scratch: head | entry head | selbad[n] | selloc[n] | spart[2 * selection workgroups]; the per-entry
  // records, sized once the entries are counted, live in the ctx's second scratch
  const uint32_t sblocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_ehead = cv.add(STEP_HEAD_SLOT), o_bad = cv.add((size_t)n * 4), o_loc = cv.add((size_t)n * 8),
               o_spart = cv.add((size_t)sblocks * 16);
  if (int st = step_begin(c, cv.size(), 2 * STEP_HEAD_SLOT, 0, 0)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EcscanArgs a{};
  a.ready = d_ready;
  a.sel = d_sel;
  a.n = n;
  a.G = G;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.data = (const uint8_t *)d_data;
  a.data_len_total = data_len_total;
  a.scan = d_scan;
  a.reqs = d_reqs;
  a.applied = d_applied;
  a.head = (EleadHead *)base;
  a.ehead = (EleadHead *)(base + o_ehead);
  a.selbad = (uint32_t *)(base + o_bad);
  a.selloc = (unsigned long long *)(base + o_loc);
  a.spart = (unsigned long long *)(base + o_spart);
  hipLaunchKernelGGL(k_cscan_sel, dim3(sblocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.spart, sblocks, a.head);
  EleadHead h[2];                                    // the committed entries; the requests
  if (int st = step_decide(c, base, 1, h)) return st;
  if (int st = step_status(h[0], false, 0, 0)) return st;
  // each selection's range lies inside d_ents, but ranges may coincide: the lanes are 32-bit ordinals
  if (h[0].n_msgs >= 0x7fffffffull) return EWAL_E_INVAL;
  a.T = h[0].n_msgs;
  const uint32_t eblocks = grid_for(a.T, 256);
  if (a.T) {
    Carve ev;
    const size_t o_rec = ev.add((size_t)a.T * sizeof(EcscanRec)), o_pos = ev.add((size_t)a.T * 8),
                 o_epart = ev.add((size_t)eblocks * 16);
    EW_CHECK(c->lcompact_stage.ensure(ev.size()));
    uint8_t *eb = c->lcompact_stage.as<uint8_t>();
    a.erec = (EcscanRec *)(eb + o_rec);
    a.epos = (unsigned long long *)(eb + o_pos);
    a.epart = (unsigned long long *)(eb + o_epart);
    hipLaunchKernelGGL(k_cscan_decode, dim3(eblocks), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_cscan_count, dim3(eblocks), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.epart, eblocks, a.ehead);
    // the decision point: the decode's flag word lies in the first head, the requests in the second
    if (int st = step_decide(c, base, 2, h)) return st;
    if (int st = step_status(h[0], d_reqs, h[1].n_msgs, reqs_cap)) return st;
    a.R = h[1].n_msgs;
    if (d_reqs)
      hipLaunchKernelGGL(k_cscan_emit<true>, dim3(eblocks), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL(k_cscan_emit<false>, dim3(eblocks), dim3(256), 0, c->stream, a);
  }
  hipLaunchKernelGGL(k_cscan_rows, dim3(sblocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_reqs) *n_reqs = a.R;
  if (n_entries) *n_entries = a.T;
  return EWAL_OK;
}

int econf_gate_batch_device(ewal_ctx *c, const elead_group *d_groups, const econf_state *d_cstate, uint64_t G,
                            const void *d_recs, uint64_t n, uint32_t rec_bytes, uint32_t from_word,
                            econf_gate_result *d_res, void *d_pass, uint64_t pass_cap, emsg_out *d_msgs,
                            uint64_t msgs_cap, uint64_t *n_pass, uint64_t *n_msgs) {
  if (n_pass) *n_pass = 0;
  if (n_msgs) *n_msgs = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (rec_bytes != 48 && rec_bytes != 64 && rec_bytes != 96) return EWAL_E_INVAL;
  if (from_word != ECONF_FROM_SELF && (from_word < 1 || from_word >= rec_bytes / 8)) return EWAL_E_INVAL;
  if ((d_pass == nullptr) != (d_msgs == nullptr)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_cstate || !d_recs || !d_res) return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_cstate, d_recs, d_res, d_pass, d_msgs})) return EWAL_E_INVAL;
  if (d_pass) {
    const uintptr_t r0 = (uintptr_t)d_recs, r1 = r0 + (uintptr_t)n * rec_bytes, p0 = (uintptr_t)d_pass,
                    p1 = p0 + (uintptr_t)std::min(pass_cap, n) * rec_bytes;
    if (r0 < p1 && p0 < r1) return EWAL_E_INVAL;
  }
  // scratch: head | message head | rec[n] | ppart[2 * workgroups] | mpart[2 * workgroups]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_mhead = cv.add(STEP_HEAD_SLOT), o_rec = cv.add((size_t)n * sizeof(EgateRec)),
               o_ppart = cv.add((size_t)blocks * 16), o_mpart = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), 2 * STEP_HEAD_SLOT, 0, 0)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EgateArgs a{};
  a.groups = d_groups;
  a.cstate = d_cstate;
  a.G = G;
  a.recs = (const uint8_t *)d_recs;
  a.n = n;
  a.rec_bytes = rec_bytes;
  a.from_word = from_word;
  a.res = d_res;
  a.pass = (uint8_t *)d_pass;
  a.msgs = d_msgs;
  a.head = (EleadHead *)base;
  a.mhead = (EleadHead *)(base + o_mhead);
  a.rec = (EgateRec *)(base + o_rec);
  a.ppart = (unsigned long long *)(base + o_ppart);
  a.mpart = (unsigned long long *)(base + o_mpart);
  hipLaunchKernelGGL(k_gate_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.ppart, blocks, a.head);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.mpart, blocks, a.mhead);
  EleadHead h;                                       // n_msgs: the copies, n_committed: the messages
  if (int st = step_decide(c, base, 1, &h)) return st;
  const bool emit = d_pass != nullptr;
  if (int st = step_status(h, emit, h.n_msgs, pass_cap)) return st;
  if (int st = step_status(h, emit, h.n_committed, msgs_cap)) return st;
  if (emit)
    hipLaunchKernelGGL(k_gate_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(k_gate_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  if (int st = step_end(c)) return st;
  if (n_pass) *n_pass = h.n_msgs;
  if (n_msgs) *n_msgs = h.n_committed;
  return EWAL_OK;
}

uint32_t enode_req_size(void) { return sizeof(enode_req); }
uint32_t enode_peer_size(void) { return sizeof(enode_peer); }
uint32_t enode_result_size(void) { return sizeof(enode_result); }

static_assert(sizeof(enode_req) == 128 && sizeof(enode_peer) == 32 && sizeof(enode_result) == 48 &&
                  sizeof(EnodeRec) == 48 && offsetof(enode_req, ents_first) == 24 && offsetof(enode_req, n_src) == 48 &&
                  offsetof(enode_req, hs_term) == 64 && offsetof(enode_req, snap) == 88 &&
                  offsetof(enode_result, nlog) == 8 && offsetof(enode_result, data_first) == 40 &&
                  offsetof(econf_state, removed) == 8 && offsetof(eready_state, snapi) == 40,
              "enode layout");
int enode_batch_device(ewal_ctx *c, elead_group *d_groups, elead_prop_state *d_pstate, evote_state *d_vstate,
                       eready_state *d_rstate, econf_state *d_cstate, elead_snap *d_snaps, uint64_t G,
                       ewal_entry *d_ents, uint64_t n_ents_total, const ewal_entry *d_src, uint64_t n_src_total,
                       const elead_snap *d_in_snaps, uint64_t n_in_snaps, const uint64_t *d_u64, uint64_t n_u64,
                       const enode_peer *d_peers, uint64_t n_peers_total, const uint8_t *d_ctx, uint64_t ctx_len,
                       uint8_t *d_data, uint64_t data_base, uint64_t data_cap, const enode_req *d_reqs, uint64_t n,
                       enode_result *d_res, uint64_t *n_data, uint64_t *n_copied, uint64_t *n_built) {
  if (n_data) *n_data = 0;
  if (n_copied) *n_copied = 0;
  if (n_built) *n_built = 0;
  if (!step_args_ok(c, n, G)) return EWAL_E_INVAL;
  if (n == 0) return EWAL_OK;
  if (!d_groups || !d_pstate || !d_vstate || !d_rstate || !d_cstate || !d_snaps || !d_reqs || !d_res ||
      (n_ents_total && !d_ents) || (n_src_total && !d_src) || (n_in_snaps && !d_in_snaps) || (n_u64 && !d_u64) ||
      (n_peers_total && !d_peers) || (ctx_len && !d_ctx))
    return EWAL_E_INVAL;
  if (!aligned(15, {d_groups, d_pstate, d_vstate, d_rstate, d_cstate, d_snaps, d_in_snaps, d_peers, d_reqs, d_res}) ||
      !aligned(7, {d_ents, d_src, d_u64}))
    return EWAL_E_INVAL;
  // scratch: head | bytes head | peers head | claim[G] | rec[n] | cpart | dpart | ppart [2 * workgroups each]
  const uint32_t blocks = grid_for(n, 256);
  Carve cv;
  cv.add(STEP_HEAD_SLOT);
  const size_t o_dhead = cv.add(STEP_HEAD_SLOT), o_phead = cv.add(STEP_HEAD_SLOT), o_claim = cv.add((size_t)G * 4),
               o_rec = cv.add((size_t)n * sizeof(EnodeRec)), o_cpart = cv.add((size_t)blocks * 16),
               o_dpart = cv.add((size_t)blocks * 16), o_ppart = cv.add((size_t)blocks * 16);
  if (int st = step_begin(c, cv.size(), 3 * STEP_HEAD_SLOT, o_claim, G)) return st;
  uint8_t *base = c->lstep.as<uint8_t>();
  EnodeArgs a{};
  a.groups = d_groups;
  a.pstate = d_pstate;
  a.vstate = d_vstate;
  a.rstate = d_rstate;
  a.cstate = d_cstate;
  a.snaps = d_snaps;
  a.G = G;
  a.ents = d_ents;
  a.n_ents_total = n_ents_total;
  a.src = d_src;
  a.n_src_total = n_src_total;
  a.in_snaps = d_in_snaps;
  a.n_in_snaps = n_in_snaps;
  a.u64 = d_u64;
  a.n_u64 = n_u64;
  a.peers = d_peers;
  a.n_peers_total = n_peers_total;
  a.ctx = d_ctx;
  a.ctx_len = ctx_len;
  a.data = d_data;
  a.data_base = data_base;
  a.in = d_reqs;
  a.n = n;
  a.res = d_res;
  a.head = (EleadHead *)base;
  a.dhead = (EleadHead *)(base + o_dhead);
  a.phead = (EleadHead *)(base + o_phead);
  a.claim = (uint32_t *)(base + o_claim);
  a.rec = (EnodeRec *)(base + o_rec);
  a.cpart = (unsigned long long *)(base + o_cpart);
  a.dpart = (unsigned long long *)(base + o_dpart);
  a.ppart = (unsigned long long *)(base + o_ppart);
  a.blocks = blocks;
  hipLaunchKernelGGL(k_node_count, dim3(blocks), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.cpart, blocks, a.head);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.dpart, blocks, a.dhead);
  hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(256), 0, c->stream, a.ppart, blocks, a.phead);
  EleadHead h[3];                                    // the copied entries and built requests; the bytes; the peers
  if (int st = step_decide(c, base, 3, h)) return st;
  if (int st = step_status(h[0], d_data, h[1].n_msgs, data_cap)) return st;
  // the lanes of the copy and marshal passes are 32-bit workgroup ordinals
  if (h[0].n_msgs >= 0x7fffffffull * 256 || h[2].n_msgs >= 0x7fffffffull * 256) return EWAL_E_INVAL;
  if (d_data) {
    hipLaunchKernelGGL(k_node_apply<true>, dim3(blocks), dim3(256), 0, c->stream, a);
    if (h[0].n_msgs) {
      a.n_work = h[0].n_msgs;
      hipLaunchKernelGGL(k_node_copy, dim3(grid_for(a.n_work, 256)), dim3(256), 0, c->stream, a);
    }
    if (h[2].n_msgs) {
      a.n_work = h[2].n_msgs;
      hipLaunchKernelGGL(k_node_marshal, dim3(grid_for(a.n_work, 256)), dim3(256), 0, c->stream, a);
    }
  } else {
    hipLaunchKernelGGL(k_node_apply<false>, dim3(blocks), dim3(256), 0, c->stream, a);
  }
  if (int st = step_end(c)) return st;
  if (n_data) *n_data = h[1].n_msgs;
  if (n_copied) *n_copied = h[0].n_msgs;
  if (n_built) *n_built = h[0].n_committed;
  return EWAL_OK;
}

int ewal_batch_entries_device(ewal_ctx *c, const ewal_entry **d_ents, uint64_t *n_total) {
  if (!c || !d_ents || !n_total || !c->bents_valid) return EWAL_E_INVAL;
  uint64_t end = 0;
  for (size_t s = 0; s < c->bnents.size(); ++s) end = std::max(end, c->bent_first[s] + c->bnents[s]);
  *d_ents = end ? c->bents.as<ewal_entry>() : nullptr;
  *n_total = end;
  return EWAL_OK;
}

int enode_reqs_from_batch(ewal_ctx *c, const ewal_result *res, uint64_t n_shards, const uint64_t *shard_off,
                          enode_req *h_reqs) {
  if (!c || !c->bents_valid || n_shards != c->bnents.size() || (n_shards && (!res || !shard_off || !h_reqs)))
    return EWAL_E_INVAL;
  for (uint64_t s = 0; s < n_shards; ++s) {
    enode_req &r = h_reqs[s];
    const bool ok = res[s].status == EWAL_OK && res[s].n_unrec == 0;
    r.group = s;
    r.kind = ok ? 1 : 0;
    r.src_first = c->bent_first[s];
    r.n_src = c->bnents[s];
    r.data_delta = shard_off[s];
    r.hs_term = res[s].has_state ? res[s].state_term : 0;
    r.hs_vote = res[s].has_state ? res[s].state_vote : 0;
    r.hs_commit = res[s].has_state ? res[s].state_commit : 0;
    r.pad[0] = r.pad[1] = r.pad[2] = r.pad[3] = 0;
  }
  return EWAL_OK;
}
