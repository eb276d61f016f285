"""Host-only part of the asynchronous frontier (`csrc/ai_flow_host.h`, compiled here with g++ under the address and undefined-behaviour
sanitizers; no GPU, nothing loaded into Python): the layouts of the tables a harvest wave keeps in pinned host memory against the
expressions `Flow` spelled out by hand before they had one definition, the header checks of a packed history row, the first-fit
allocator of stable task indices against a bitmap, and the rules that turn a harvested segment into children and groups
(DESIGN.md section 29)."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = textwrap.dedent(r'''
    #include "ai_flow_host.h"
    #include <cstdio>
    #include <cstring>
    #include <random>
    #include <set>
    #include <string>

    #define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

    // the pinned buffers as the frontier has always sized them
    static const size_t HIST_BYTES = (size_t)16 << 20, COEF_BYTES = (size_t)8 << 20;

    struct Field { size_t off, len; bool dbl; };
    static int fields_ok(const std::vector<Field>& f, size_t size) {
      size_t end = 0;
      for (const Field& x : f) {
        CHECK(x.off >= end);                 // disjoint and in order
        CHECK(!x.dbl || x.off % 8 == 0);     // doubles are 8-byte aligned
        end = x.off + x.len;
      }
      CHECK(end == size);                    // the reported size is the end of the last field
      return 0;
    }

    static int layouts() {
      std::vector<double> store((size_t)512 * (3 * 4000 + 4) + 16);   // the largest table of the grid: 512 history rows of mp = 4000
      double* const cb = store.data();
      char* const base = (char*)cb;
      CHECK((size_t)base % 16 == 0);
      for (size_t nA : {1, 2, 3, 5, 511, 512}) {
        // {split[nA], ntrue[nA], kstar[nA]} int32, padded to 16 bytes, then mcut[nA], resid[nA], rtrue[nA] double
        const WaveResults R(nA);
        const size_t dbl0 = ((size_t)3 * nA * sizeof(int32_t) + 15) & ~(size_t)15;
        CHECK((char*)R.split(base) - base == 0);
        CHECK((char*)R.ntrue(base) - base == (ptrdiff_t)(nA * 4));
        CHECK((char*)R.kstar(base) - base == (ptrdiff_t)(2 * nA * 4));
        CHECK((char*)R.mcut(base) - base == (ptrdiff_t)dbl0);
        CHECK((char*)R.resid(base) - base == (ptrdiff_t)(dbl0 + nA * 8));
        CHECK((char*)R.rtrue(base) - base == (ptrdiff_t)(dbl0 + 2 * nA * 8));
        CHECK(R.bytes() == dbl0 + 3 * nA * 8);
        if (fields_ok({{(size_t)((char*)R.split(base) - base), nA * 4, false}, {(size_t)((char*)R.ntrue(base) - base), nA * 4, false},
                       {(size_t)((char*)R.kstar(base) - base), nA * 4, false}, {(size_t)((char*)R.mcut(base) - base), nA * 8, true},
                       {(size_t)((char*)R.resid(base) - base), nA * 8, true}, {(size_t)((char*)R.rtrue(base) - base), nA * 8, true}}, R.bytes())) return 1;
        CHECK(RES_WAVE + R.bytes() <= RES_SLAB_TABLE);
        for (size_t mp : {1, 2, 63, 4000}) for (int warm = 0; warm < 2; ++warm) {
          // {cu[nA], theta[nA], m[nA] in a row of nA doubles, coef[nA][mp]} + warm: {cu2[nA], coef2[nA][mp]}
          const CoefTable C(nA, mp, warm != 0);
          CHECK(C.cu(cb) == cb);
          CHECK(C.theta(cb) == cb + nA);
          CHECK((char*)C.m(cb) == (char*)(cb + 2 * nA));
          CHECK(C.coef(cb) == cb + 3 * nA);
          CHECK(C.cu2(cb) == cb + 3 * nA + nA * mp);
          CHECK(C.coef2(cb) == cb + 3 * nA + nA * mp + nA);
          for (size_t i : {(size_t)0, nA / 2, nA - 1}) {
            CHECK(C.coef(cb, i) == cb + 3 * nA + i * mp);
            CHECK(C.coef2(cb, i) == cb + 3 * nA + nA * mp + nA + i * mp);
          }
          CHECK(C.coef((const double*)cb, nA - 1) == cb + 3 * nA + (nA - 1) * mp);   // the same table over a read-only base
          CHECK(C.doubles() == 3 * nA + nA * mp + (warm ? nA + nA * mp : 0));         // the upload
          CHECK(C.bytes() == C.doubles() * 8);
          CHECK(C.top_doubles() == 3 * nA + nA * mp);                                   // the guard log's copy
          std::vector<Field> f = {{0, nA * 8, true}, {(size_t)(C.theta(cb) - cb) * 8, nA * 8, true}, {(size_t)((char*)C.m(cb) - base), nA * 8, false},
                                  {(size_t)(C.coef(cb) - cb) * 8, nA * mp * 8, true}};   // (m: int32 in a row that is nA doubles wide)
          if (warm) f.push_back({(size_t)(C.cu2(cb) - cb) * 8, nA * 8, true}), f.push_back({(size_t)(C.coef2(cb) - cb) * 8, nA * mp * 8, true});
          if (fields_ok(f, C.bytes())) return 1;
          // history rows: {theta, resid, m, checksum, a[mp], b[mp], g[mp]}
          const HistRows H(mp);
          CHECK(H.pitch() == 3 * mp + 4 && FK_HIST_HEAD == 4);
          CHECK(H.row(cb, nA - 1) == cb + (nA - 1) * (3 * mp + 4));
          const double* row = H.row(cb, nA - 1);
          CHECK(H.a(row) == row + 4 && H.b(row) == row + 4 + mp && H.g(row) == row + 4 + 2 * mp);
          CHECK(H.doubles(nA) == nA * (3 * mp + 4) && H.bytes(nA) == nA * (3 * mp + 4) * 8);
          // the capacity of a wave: the inequality start_wave wrote out
          const size_t k = nA;
          const bool too_big = k * ((size_t)3 * mp + 4) * sizeof(double) > HIST_BYTES || ((warm ? 2 : 1) * k * (size_t)mp + 4 * k) * sizeof(double) > COEF_BYTES;
          CHECK(wave_fits(k, mp, warm != 0) == !too_big);
        }
      }
      // ... and up to the first k that no longer fits
      for (size_t mp : {4000, 2000}) for (int warm = 0; warm < 2; ++warm) {
        size_t k = 1;
        for (;; ++k) {
          const bool too_big = k * ((size_t)3 * mp + 4) * sizeof(double) > HIST_BYTES || ((warm ? 2 : 1) * k * (size_t)mp + 4 * k) * sizeof(double) > COEF_BYTES;
          CHECK(wave_fits(k, mp, warm != 0) == !too_big);
          if (too_big) break;
        }
        CHECK(k > 1 && wave_fits(k - 1, mp, warm != 0) && !wave_fits(k, mp, warm != 0) && !wave_fits(k + 1, mp, warm != 0));
        printf("mp %zu warm %d: first k that does not fit %zu\n", mp, warm, k);
      }
      CHECK(PIN_HIST == HIST_BYTES && PIN_COEF == COEF_BYTES && WAVE_MAX_SEGS == 512);
      CHECK(COEF_DEV_DOUBLES == COEF_BYTES / sizeof(double) + 4 * 512 + 64);
      CHECK(COEF_DEV_DOUBLES * 8 >= COEF_BYTES);
      // the regions and the named places of the result region
      CHECK(PIN_OFF_STATUS == PIN_UP && PIN_OFF_RES == PIN_UP + PIN_STATUS && PIN_OFF_HIST == PIN_UP + PIN_STATUS + PIN_RES);
      CHECK(PIN_OFF_COEF == PIN_UP + PIN_STATUS + PIN_RES + PIN_HIST && PIN_TOTAL == PIN_OFF_COEF + PIN_COEF);
      CHECK((char*)res_comp_total(base) == base && (char*)res_progress(base) == base + 32 && res_wave(base) == base + 64);
      CHECK((char*)res_child_comps(base) == base + 64 && (char*)res_slab_table(base) == base + PIN_RES / 2);
      for (size_t n : {(size_t)1, (size_t)1000, (PIN_RES / 2 - 64) / 4, (PIN_RES / 2 - 64) / 4 + 1})
        CHECK(res_child_comps_fit(n) == !(n * sizeof(int32_t) + 64 > PIN_RES / 2));
      const CompTable T(7);
      CHECK((char*)T.troot(base) == base && T.tsize(base) == (int32_t*)base + 7 && T.bytes() == 56 && T.fits_pinned());
      CHECK(CompTable(HIST_BYTES / 8).fits_pinned() && !CompTable(HIST_BYTES / 8 + 1).fits_pinned());
      return 0;
    }

    static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
    static double from_bits(unsigned long long u) { double v; memcpy(&v, &u, 8); return v; }
    // a row as fk_pack_hist documents it: the checksum is the sum of the bit patterns of theta, resid, a / b / g[0..m) and m
    static void seal(const HistRows& H, double* row, int m) {
      unsigned long long s = bits(row[0]) + bits(row[1]) + (unsigned long long)(long long)m;
      for (int j = 0; j < m; ++j) s += bits(row[4 + j]) + bits(row[4 + H.mp + j]) + bits(row[4 + 2 * H.mp + j]);
      row[2] = (double)m;
      row[3] = from_bits(s);
    }
    static int history_rows() {
      std::mt19937_64 rng(11);
      std::uniform_real_distribution<double> U(-1.0, 1.0);
      for (int mp : {1, 5, 63}) for (int m : {1, mp / 2 + 1, mp}) {
        const HistRows H((size_t)mp);
        std::vector<double> store(H.doubles(3));
        for (double& v : store) v = U(rng);
        double* row = store.data() + H.pitch();   // the middle row of three
        seal(H, row, m);
        CHECK(H.accepts(row, m) && H.m_matches(row, m) && H.sum_matches(row, m));
        CHECK(H.theta(row) == row[0] && H.resid(row) == row[1] && H.m_dev(row) == (double)m);
        // any single bit of the header, of a, b or g below m
        std::vector<int> words = {0, 1, 2, 3};
        for (int j = 0; j < m; ++j) words.push_back(4 + j), words.push_back(4 + mp + j), words.push_back(4 + 2 * mp + j);
        for (int w : words) for (int b = 0; b < 64; ++b) {
          const double keep = row[w];
          row[w] = from_bits(bits(keep) ^ (1ull << b));
          CHECK(!H.accepts(row, m));
          CHECK(w == 2 ? !H.m_matches(row, m) : (H.m_matches(row, m) && !H.sum_matches(row, m)));
          row[w] = keep;
        }
        CHECK(H.accepts(row, m));
        // entries at or beyond m do not matter
        for (int j = m; j < mp; ++j) row[4 + j] = U(rng), row[4 + mp + j] = NAN, row[4 + 2 * mp + j] = U(rng);
        CHECK(H.accepts(row, m));
        // the device froze the segment at another size of T than the host knows: a row sealed for its own m, and a stored m alone
        if (m < mp) {
          seal(H, row, m + 1);
          CHECK(!H.accepts(row, m) && !H.m_matches(row, m) && H.accepts(row, m + 1));
          seal(H, row, m);
        }
        row[2] = (double)(m + 1);
        CHECK(!H.accepts(row, m) && !H.accepts(row, m + 1 <= mp ? m + 1 : m));
        row[2] = (double)m;
        CHECK(H.accepts(row, m));
      }
      return 0;
    }

    static int range_alloc() {
      for (int cap : {1, 64, 257}) {
        std::mt19937 rng(1234 + cap);
        RangeAlloc ra;
        ra.init(cap);
        std::vector<char> used(cap, 0);
        std::vector<std::pair<int, int>> live;
        for (int it = 0; it < 4000; ++it) {
          if (live.empty() || rng() % 100 < 55) {
            const int n = 1 + (int)(rng() % (rng() % 4 ? 9 : 70));
            int want = -1;
            for (int b = 0, run = 0; b < cap && want < 0; ++b) {   // brute-force first fit
              run = used[b] ? 0 : run + 1;
              if (run == n) want = b - n + 1;
            }
            const int got = ra.alloc(n);
            CHECK(got == want);
            if (got >= 0) {
              for (int b = got; b < got + n; ++b) used[b] = 1;
              live.push_back({got, n});
            }
          } else {
            const size_t i = rng() % live.size();
            ra.release(live[i].first, live[i].second);
            for (int b = live[i].first; b < live[i].first + live[i].second; ++b) used[b] = 0;
            live[i] = live.back();
            live.pop_back();
          }
        }
        for (auto& r : live) ra.release(r.first, r.second);
        CHECK(ra.fr.size() == 1 && ra.fr.begin()->first == 0 && ra.fr.begin()->second == cap);
        CHECK(ra.alloc(cap) == 0 && ra.alloc(1) == -1);
      }
      return 0;
    }

    static bool same(double a, double b) { return bits(a) == bits(b); }
    // every field of a child: those the rule sets, and the defaults of all others
    static bool child_is(const FSeg& c, int g0, int n, int chunk, int par, bool binary, int vdelta, int warm_n, int restarts, double prev_true, double front,
                         double path) {
      return c.g0 == g0 && c.n == n && c.chunk == chunk && c.par == par && c.binary_child == binary && c.vdelta == vdelta && c.warm_n == warm_n &&
             c.restarts == restarts && same(c.prev_true, prev_true) && same(c.front, front) && same(c.path, path) && c.slot == -1 && c.f0 == -1 && c.c0 == -1 &&
             c.t0 == 0 && c.cap == 0 && c.m == 0 && c.aux == 0 && !c.frozen && c.pca == 0;
    }
    static bool leaf_is(const FLeaf& l, int g0, double front) { return l.g0 == g0 && same(l.front, front) && std::isnan(l.cost); }
    static FSeg pool_seg(int g0, int n, double front, double path) {   // a harvested segment: everything a child must NOT inherit is set
      FSeg s;
      s.g0 = g0, s.n = n, s.chunk = 3, s.par = 1, s.slot = 5, s.t0 = 77, s.cap = 40, s.f0 = 8, s.c0 = 2, s.m = 31, s.aux = 6, s.frozen = true;
      s.binary_child = true, s.vdelta = -9, s.warm_n = 640, s.pca = 4, s.restarts = 1, s.prev_true = 0.5, s.front = front, s.path = path;
      return s;
    }

    static int child_rules() {
      std::vector<FSeg> ch;
      std::vector<FLeaf> lv;
      const double ninf = -INFINITY;
      // ---- solved again: the same rows, graph and heights; one more restart; the ancestor's warm vector
      FSeg s = pool_seg(100, 50, 0.02, 0.05);
      child_solve_again(s, 3e-5, ch);
      CHECK(ch.size() == 1 && child_is(ch[0], 100, 50, 3, 1, false, -9, 640, 2, 3e-5, 0.02, 0.05));
      FSeg root;
      root.g0 = 0, root.n = 400, root.binary_child = true;
      ch.clear();
      child_solve_again(root, 1e-3, ch);
      CHECK(child_is(ch[0], 0, 400, 0, 0, false, 0, 0, 1, 1e-3, ninf, ninf));
      // ---- a Fiedler cut.  n_orig = 1000: a side continues from 11 rows on (10 / 1000 is not ABOVE 1 %)
      ch.clear();
      CutSides r = children_of_cut(s, 39, 0.03, 1000, ch, lv);   // 39 | 11, a cut cheaper than an ancestor's: path stays 0.05
      CHECK(r.ok && r.na == 39 && r.nb == 11 && r.contA && r.contB && lv.empty() && ch.size() == 2);
      CHECK(child_is(ch[0], 100, 39, 3, 0, true, -9, 50, 0, 0.0, 0.02, 0.05));
      CHECK(child_is(ch[1], 139, 11, 3, 0, true, -9, 50, 0, 0.0, 0.05, 0.05));
      ch.clear();
      r = children_of_cut(s, 40, 0.08, 1000, ch, lv);            // 40 | 10: B is a group; the cut is the dearest so far
      CHECK(r.ok && r.contA && !r.contB && ch.size() == 1 && lv.size() == 1);
      CHECK(child_is(ch[0], 100, 40, 3, 0, true, -9, 50, 0, 0.0, 0.02, 0.08) && leaf_is(lv[0], 140, 0.08));
      ch.clear(), lv.clear();
      r = children_of_cut(s, 10, 0.08, 1000, ch, lv);            // 10 | 40: A is a group in front of which the parent's boundary stays
      CHECK(r.ok && !r.contA && r.contB && ch.size() == 1 && lv.size() == 1);
      CHECK(leaf_is(lv[0], 100, 0.02) && child_is(ch[0], 110, 40, 3, 0, true, -9, 50, 0, 0.0, 0.08, 0.08));
      ch.clear(), lv.clear();
      r = children_of_cut(s, 2, 0.03, 20, ch, lv);               // 2 | 48 of a 20-point chunk: two rows are never split
      CHECK(r.ok && !r.contA && r.contB && leaf_is(lv[0], 100, 0.02));
      ch.clear(), lv.clear();
      r = children_of_cut(pool_seg(100, 13, 0.02, 0.05), 3, 0.03, 1000, ch, lv);   // 3 | 10: both sides groups
      CHECK(r.ok && !r.contA && !r.contB && ch.empty() && lv.size() == 2 && leaf_is(lv[0], 100, 0.02) && leaf_is(lv[1], 103, 0.05));
      ch.clear(), lv.clear();
      r = children_of_cut(root, 5, 0.2, 400, ch, lv);            // a root (-inf heights), n_orig = 400: 5 rows continue, 4 would not
      CHECK(r.ok && r.contA && r.contB && child_is(ch[0], 0, 5, 0, 1, true, 0, 400, 0, 0.0, ninf, 0.2) && child_is(ch[1], 5, 395, 0, 1, true, 0, 400, 0, 0.0, 0.2, 0.2));
      ch.clear(), lv.clear();
      r = children_of_cut(root, 4, 0.2, 400, ch, lv);
      CHECK(r.ok && !r.contA && r.contB && leaf_is(lv[0], 0, ninf) && child_is(ch[0], 4, 396, 0, 1, true, 0, 400, 0, 0.0, 0.2, 0.2));
      ch.clear(), lv.clear();
      for (int nt : {0, 50, -1, 51}) {                            // an empty side is reported, nothing is appended
        r = children_of_cut(s, nt, 0.03, 1000, ch, lv);
        CHECK(!r.ok && r.na == nt && r.nb == 50 - nt && ch.empty() && lv.empty());
      }
      // ---- a split into components.  The wave's table: a run of another segment in front and behind
      {
        const int32_t troot[] = {10, 20, 200, 212, 215, 230, 240}, tsize[] = {10, 5, 12, 3, 15, 10, 1};
        int32_t cont[7] = {0, 0, 0, 0, 0, 0, 0};
        FSeg m = pool_seg(200, 30, 0.07, 0.01);
        m.binary_child = true;
        size_t ti = 2;
        CompSplit c = children_of_components(m, troot, tsize, 7, ti, 1000, cont, ch, lv);   // 12 | 3 | 15 rows: the middle one is a group
        CHECK(c.status == COMP_OK && c.covered == 30 && ti == 5 && ch.size() == 2 && lv.size() == 1);
        CHECK(cont[2] == 1 && cont[3] == 0 && cont[4] == 1 && cont[0] + cont[1] + cont[5] + cont[6] == 0);
        CHECK(child_is(ch[0], 200, 12, 3, 0, false, -9, 640, 0, 0.0, 0.07, 0.01));     // the first inherits the parent's front
        CHECK(leaf_is(lv[0], 212, 0.01) && child_is(ch[1], 215, 15, 3, 0, false, -9, 640, 0, 0.0, 0.01, 0.01));
        ch.clear(), lv.clear();
        FSeg r0 = root;                                           // a root that falls apart: the cut between components costs 0
        r0.g0 = 200, r0.n = 30;
        ti = 2;
        c = children_of_components(r0, troot, tsize, 7, ti, 1000, cont, ch, lv);
        CHECK(c.status == COMP_OK && child_is(ch[0], 200, 12, 0, 1, false, 0, 0, 0, 0.0, ninf, 0.0) && leaf_is(lv[0], 212, 0.0) &&
              child_is(ch[1], 215, 15, 0, 1, false, 0, 0, 0, 0.0, 0.0, 0.0));
        ch.clear(), lv.clear();
        FSeg first_small = pool_seg(10, 15, 0.3, -0.5);           // 10 | 5 rows: the first component is the group, with the parent's front
        ti = 0;
        c = children_of_components(first_small, troot, tsize, 7, ti, 1000, cont, ch, lv);
        CHECK(c.status == COMP_OK && ti == 2 && leaf_is(lv[0], 10, 0.3) && lv.size() == 2 && leaf_is(lv[1], 20, 0.0) && ch.empty());
        lv.clear();
        // tables that do not tile the segment
        ti = 1;                                                    // a component that starts in front of the segment
        CHECK(children_of_components(m, troot, tsize, 7, ti, 1000, cont, ch, lv).status == COMP_NO_TILE);
        const int32_t over[] = {12, 3, 16}, zero[] = {12, 0, 15}, few[] = {12, 3, 14};
        ti = 0;
        CHECK(children_of_components(m, troot + 2, over, 3, ti, 1000, cont, ch, lv).status == COMP_NO_TILE);   // runs past its end
        ti = 0;
        CHECK(children_of_components(m, troot + 2, zero, 3, ti, 1000, cont, ch, lv).status == COMP_NO_TILE);   // an empty component
        ti = 0;
        c = children_of_components(m, troot + 2, few, 3, ti, 1000, cont, ch, lv);                             // a row is missing
        CHECK(c.status == COMP_SHORT && c.covered == 29);
        ti = 3;
        c = children_of_components(m, troot + 2, tsize + 2, 3, ti, 1000, cont, ch, lv);                       // no run at all
        CHECK(c.status == COMP_SHORT && c.covered == 0);
        ch.clear(), lv.clear();
      }
      // ---- seeded random parents: children and groups tile the parent exactly once, in increasing order within each list
      std::mt19937 rng(99);
      for (int it = 0; it < 3000; ++it) {
        FSeg p = pool_seg((int)(rng() % 5000), 2 + (int)(rng() % 300), 0.01 * (rng() % 9), 0.01 * (rng() % 9));
        const int64_t n_orig = 1 + rng() % 3000;
        std::vector<int> starts, sizes;
        std::vector<int32_t> contv;
        ch.clear(), lv.clear();
        if (it & 1) {
          const int nt = 1 + (int)(rng() % (p.n - 1));
          const CutSides q = children_of_cut(p, nt, 0.001 * (rng() % 100), n_orig, ch, lv);
          CHECK(q.ok);
          starts = {p.g0, p.g0 + nt}, sizes = {nt, p.n - nt};
          contv = {q.contA, q.contB};
        } else {
          std::vector<int32_t> tr, ts;
          for (int o = 0; o < p.n;) {
            const int c = 1 + (int)(rng() % (unsigned)std::min(p.n - o, 1 + (int)(rng() % 60)));
            tr.push_back(p.g0 + o), ts.push_back(c), starts.push_back(p.g0 + o), sizes.push_back(c);
            o += c;
          }
          tr.push_back(p.g0 + p.n), ts.push_back(7);   // the next segment's first component
          contv.assign(tr.size(), 0);
          size_t ti = 0;
          const CompSplit q = children_of_components(p, tr.data(), ts.data(), tr.size(), ti, n_orig, contv.data(), ch, lv);
          CHECK(q.status == COMP_OK && q.covered == p.n && ti + 1 == tr.size() && contv.back() == 0);
          contv.pop_back();
        }
        size_t ci = 0, li = 0;
        for (size_t k = 0; k < starts.size(); ++k) {   // piece k is the next child or the next group, as the flag says, and nothing else is left
          CHECK(contv[k] == (eligible(sizes[k], n_orig, 0.01) ? 1 : 0));
          if (contv[k]) {
            CHECK(ci < ch.size() && ch[ci].g0 == starts[k] && ch[ci].n == sizes[k]);
            ++ci;
          } else {
            CHECK(li < lv.size() && lv[li].g0 == starts[k] && std::isnan(lv[li].cost));
            ++li;
          }
        }
        CHECK(ci == ch.size() && li == lv.size());
      }
      return 0;
    }

    int main(int argc, char** argv) {
      const std::string what = argc > 1 ? argv[1] : "";
      if (what == "layouts") return layouts();
      if (what == "history_rows") return history_rows();
      if (what == "range_alloc") return range_alloc();
      if (what == "child_rules") return child_rules();
      return 64;
    }
''')


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The stand-alone program: ai_flow_host.h and the standard library alone, built with the sanitizers, run as a child process."""
    d = tmp_path_factory.mktemp("host_flow")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(PROGRAM)
    csrc = os.path.join(ROOT, "autoinst_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", csrc, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, part):
    r = subprocess.run([exe, part], capture_output=True, text=True)
    assert r.returncode == 0, (part, r.returncode, r.stdout, r.stderr)
    return r.stdout


def test_the_header_needs_nothing_of_hip():
    with open(os.path.join(ROOT, "autoinst_amd", "csrc", "ai_flow_host.h")) as f:
        text = f.read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "ai_common.h" not in "".join(includes) and not any("hip" in i for i in includes), includes
    with open(os.path.join(ROOT, "autoinst_amd", "csrc", "ai_ncut_params.h")) as f:
        assert [line for line in f.read().splitlines() if line.startswith("#include")] == ["#include <stdint.h>"]


def test_wave_tables_lie_where_the_frontier_always_put_them(program):
    out = _run(program, "layouts")
    # by hand: 16 MB of histories take 174 rows of 12004 doubles (mp = 4000) or 349 of 6004 (mp = 2000); 8 MB of coefficients take
    # 131 segments of 8004 doubles (mp = 4000, warm) or 261 of 4004 (mp = 2000, warm), and more than the histories without the second vector
    for mp, warm, k in ((4000, 0, 175), (4000, 1, 132), (2000, 0, 350), (2000, 1, 262)):
        assert "mp %d warm %d: first k that does not fit %d\n" % (mp, warm, k) in out, out


def test_a_history_row_is_accepted_only_with_its_header_intact(program):
    _run(program, "history_rows")


def test_range_alloc_is_first_fit(program):
    _run(program, "range_alloc")


def test_children_and_groups_of_a_harvested_segment(program):
    _run(program, "child_rules")
