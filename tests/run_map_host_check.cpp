// Host run of the per-run un-permute map of the tiled pullback (csrc/dpr_run_map.h): run_map_encode builds the map of
// a scatter sub-chunk from (tile of each point, cursors) by the phases of scatter_wc_body, run_map_decode reads every
// sorted position back by the steps of k_unpermute_runs.  tests/test_run_map_host.py builds this file with
// -fsanitize=address,undefined and runs it as a child process.  No input.
// Every case is a sub-chunk of nloc <= S points over NT tiles, S = 2048 and S = 4096, encoded TWICE in a row on the same
// cursors (the second round starts where the first left them).  The expectation is a plain counting sort written here:
// points in ascending tile order, original order inside a tile, record slot = cursor of the tile + rank.  Checked:
//   1. a run starts at the first record of every tile and at every 64th position, the table holds the slots of a
//      segment's run starts packed to the front of the segment's 64 entries, and no other entry is written,
//   2. every position i < n_valid decodes to the owner and the record slot of the counting sort,
//   3. every position n_valid <= i < nloc decodes to "no record",
//   4. dest[] of every accepted point and the cursors after the round are those of the counting sort,
//   5. every buffer is exactly as long as the kernels may assume (owner nloc, table nloc): the sanitizer sees the rest.
// Exit status: 0 all cases pass, 1 a statement failed (named on stderr), 2 bad arguments.  `--flip-start-bit` (for the
// test of the checker itself) inverts the run-start bit of ONE owner word of every map with a record, after the
// encoder and before the decoder: statement 2 must fail.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../diffpointrasterisation.jl_amd/csrc/dpr_run_map.h"

using namespace dpr;

static bool g_flip = false;
static long long g_cases = 0, g_positions = 0;

static int fail(int statement, const char* name, int S, const char* what, long long a, long long b) {
    fprintf(stderr, "%s (S = %d): statement %d: %s (%lld, %lld)\n", name, S, statement, what, a, b);
    return 1;
}

template <int S> static int round_of(const char* name, const std::vector<int>& tile, int NT, std::vector<uint32_t>& cursor) {
    const uint32_t nloc = (uint32_t)tile.size();
    const uint32_t kUnwritten = 0xdeadbeefu;
    // the counting sort
    std::vector<uint32_t> cnt(NT, 0), off(NT, 0), ref_owner, ref_slot, ref_dest(nloc, 0);
    for (uint32_t lp = 0; lp < nloc; ++lp)
        if (tile[lp] >= 0) ++cnt[tile[lp]];
    uint32_t n_valid = 0, runs = 0;
    for (int t = 0; t < NT; ++t) {
        off[t] = n_valid;
        n_valid += cnt[t];
    }
    ref_owner.resize(n_valid);
    ref_slot.resize(n_valid);
    std::vector<uint32_t> fill(NT, 0);
    for (uint32_t lp = 0; lp < nloc; ++lp) {
        if (tile[lp] < 0) continue;
        const int t = tile[lp];
        ref_owner[off[t] + fill[t]] = lp;
        ref_slot[off[t] + fill[t]] = ref_dest[lp] = cursor[t] + fill[t];
        ++fill[t];
    }
    std::vector<uint32_t> ref_table(nloc, kUnwritten);
    for (uint32_t i = 0, j = 0; i < n_valid; ++i) {
        if (i % 64 == 0) j = 0;
        if (i % 64 == 0 || tile[ref_owner[i]] != tile[ref_owner[i - 1]]) {
            ref_table[i / 64 * 64 + j++] = ref_slot[i];
            ++runs;
        }
    }
    std::vector<uint32_t> ref_cursor(cursor);
    for (int t = 0; t < NT; ++t) ref_cursor[t] += cnt[t];
    // the map
    std::vector<uint16_t> owner(nloc, 0);
    std::vector<uint32_t> table(nloc, kUnwritten), dest(nloc, kUnwritten), lhist(NT), lrank(S);
    const uint32_t R = run_map_encode<S>(tile.data(), nloc, NT, cursor.data(), owner.data(), table.data(), dest.data(),
                                         lhist.data(), lrank.data());
    if (R != runs) return fail(1, name, S, "runs: encoder, counting sort", R, runs);
    for (uint32_t k = 0; k < nloc; ++k)
        if (table[k] != ref_table[k]) return fail(1, name, S, "table entry: index, value", k, table[k]);
    for (uint32_t lp = 0; lp < nloc; ++lp)
        if (dest[lp] != (tile[lp] >= 0 ? ref_dest[lp] : kUnwritten)) return fail(4, name, S, "dest of point", lp, dest[lp]);
    for (int t = 0; t < NT; ++t)
        if (cursor[t] != ref_cursor[t]) return fail(4, name, S, "cursor of tile after the round", t, cursor[t]);
    if (g_flip && n_valid) owner[n_valid / 2] ^= (uint16_t)kRunStart;
    // every slot the sub-chunk owns lies below P = the end of the cursors' range
    uint64_t P = 0;
    for (int t = 0; t < NT; ++t) P = cursor[t] > P ? cursor[t] : P;
    std::vector<uint32_t> slot(nloc, 0), lp(nloc, 0);
    std::vector<char> has(nloc, 0);
    static_assert(sizeof(bool) == sizeof(char), "has[] is handed over as bool");
    run_map_decode<S>(owner.data(), table.data(), nloc, P, slot.data(), lp.data(), reinterpret_cast<bool*>(has.data()));
    for (uint32_t i = 0; i < nloc; ++i) {
        if (i < n_valid) {
            if (!has[i]) return fail(2, name, S, "position decodes to no record", i, n_valid);
            if (lp[i] != ref_owner[i]) return fail(2, name, S, "owner of position", i, lp[i]);
            if (slot[i] != ref_slot[i]) return fail(2, name, S, "slot of position", i, slot[i]);
        } else if (has[i]) {
            return fail(3, name, S, "position past the records decodes to one", i, slot[i]);
        }
    }
    ++g_cases;
    g_positions += nloc;
    return 0;
}

template <int S> static int sub_chunk(const char* name, const std::vector<int>& tile, int NT, uint32_t seed) {
    // cursors as a scatter meets them: the tiles' record ranges one after the other, room for two rounds each
    // (a tile takes at most nloc records per round)
    std::mt19937 rng(seed);
    std::vector<uint32_t> cursor(NT);
    uint32_t next = rng() % 1000;
    for (int t = 0; t < NT; ++t) {
        cursor[t] = next;
        next += 2 * (uint32_t)tile.size() + rng() % 7;
    }
    if (int rc = round_of<S>(name, tile, NT, cursor)) return rc;
    return round_of<S>(name, tile, NT, cursor);
}

template <int S> static int all_cases() {
    std::vector<int> t;
    int rc = 0;
    // every point in one tile
    t.assign(S, 5);
    if ((rc = sub_chunk<S>("one tile", t, 8, 1))) return rc;
    // every point in its own tile: R = S
    t.resize(S);
    for (int i = 0; i < S; ++i) t[i] = (i * 7 + 3) % S;  // (7 is coprime to S: a permutation of the tiles)
    if ((rc = sub_chunk<S>("every point its own tile", t, S, 2))) return rc;
    // no valid point at all
    t.assign(S, -1);
    if ((rc = sub_chunk<S>("no valid point", t, 32, 3))) return rc;
    // valid and rejected alternating
    for (int i = 0; i < S; ++i) t[i] = (i & 1) ? -1 : (i / 2) % 48;
    if ((rc = sub_chunk<S>("alternating, valid first", t, 48, 4))) return rc;
    for (int i = 0; i < S; ++i) t[i] = (i & 1) ? (i / 2) % 48 : -1;
    if ((rc = sub_chunk<S>("alternating, rejected first", t, 48, 5))) return rc;
    // a single valid point, first or last
    t.assign(S, -1);
    t[0] = 17;
    if ((rc = sub_chunk<S>("single valid point, first", t, 32, 6))) return rc;
    t.assign(S, -1);
    t[S - 1] = 0;
    if ((rc = sub_chunk<S>("single valid point, last", t, 32, 7))) return rc;
    // a ragged last sub-chunk
    std::mt19937 rng(100 + S);
    for (int nloc : {1, S - 1, S}) {
        t.resize(nloc);
        for (int i = 0; i < nloc; ++i) t[i] = rng() % 10 == 0 ? -1 : (int)(rng() % 2048);
        if ((rc = sub_chunk<S>("ragged", t, 2048, 8 + (uint32_t)nloc))) return rc;
        t.assign(nloc, 0);  // (a ragged one where every position holds a record)
        if ((rc = sub_chunk<S>("ragged, one tile", t, 1, 9 + (uint32_t)nloc))) return rc;
    }
    // random sub-chunks with 1 - 4096 tiles
    for (int c = 0; c < 1000; ++c) {
        const int NT = 1 + (int)(rng() % 4096);
        const int nloc = c % 10 == 0 ? 1 + (int)(rng() % S) : S;
        const uint32_t reject = rng() % 4 == 0 ? 0 : rng() % 100;  // per cent
        const int used = rng() % 3 == 0 ? 1 + (int)(rng() % NT) : NT;  // tiles the points fall into
        t.resize(nloc);
        for (int i = 0; i < nloc; ++i) t[i] = rng() % 100 < reject ? -1 : (int)(rng() % used);
        if ((rc = sub_chunk<S>("random", t, NT, 1000 + (uint32_t)c))) return rc;
    }
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--flip-start-bit")) g_flip = true;
        else {
            fprintf(stderr, "usage: %s [--flip-start-bit]\n", argv[0]);
            return 2;
        }
    }
    for (int S : {2048, 4096}) {
        g_cases = g_positions = 0;
        const int rc = S == 2048 ? all_cases<2048>() : all_cases<4096>();
        if (rc) return rc;
        printf("S = %d: ok (%lld maps, %lld positions)\n", S, g_cases, g_positions);
    }
    return 0;
}
