// tests/native/filter_set_harness.cpp — TEST INFRASTRUCTURE.  The filter set of ipcfp_scan_events_multi
// (csrc/kernels/filter_set.h: build on the host, probe on the device) compiled for the host, as a stand-alone program:
//
//   filter_set_harness probe < text      build a set, probe keys, print what the probe finds
//   filter_set_harness slots < text      print the home slot of every key in a table of the given size
//
// Input (whitespace separated): n_specs, then per spec `key_hex(128) has_actor actor`; then n_probes, then per probe
// `key_hex(128) emitter`.  Output of `probe`, one line per probe:
//   `group compares member_spec…`   the group (-1: none), the number of full compares made, and the specs of the group's
//                                   members whose emitter filter passes, in stored order
// preceded by one line `n_slots n_groups`.  `slots`: input n_slots n_keys key_hex…, one home slot per line.
// tests/test_scan_multi.py holds the answers to a Python dict.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ipc-filecoin-proofs_amd/csrc/kernels/filter_set.h"

using namespace ipcfp;

static bool read_key(uint8_t out[64]) {
    char buf[160];
    if (std::scanf("%159s", buf) != 1 || std::strlen(buf) != 128) return false;
    for (int i = 0; i < 64; ++i) {
        unsigned v;
        if (std::sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        out[i] = uint8_t(v);
    }
    return true;
}

static void words_of(const uint8_t key[64], uint64_t w[8]) {
    for (int k = 0; k < 8; ++k) std::memcpy(&w[k], key + 8 * k, 8);  // little-endian host, like the device
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string mode = argv[1];
    if (mode == "slots") {
        unsigned n_slots, n;
        if (std::scanf("%u %u", &n_slots, &n) != 2 || n_slots == 0 || (n_slots & (n_slots - 1))) return 2;
        for (unsigned i = 0; i < n; ++i) {
            uint8_t key[64];
            uint64_t w[8];
            if (!read_key(key)) return 2;
            words_of(key, w);
            std::printf("%u\n", fs_home_slot(fs_fingerprint(w), n_slots - 1));
        }
        return 0;
    }
    if (mode != "probe") return 2;
    unsigned n;
    if (std::scanf("%u", &n) != 1 || n == 0) return 2;
    std::vector<uint8_t> keys(size_t(n) * 64), has(n);
    std::vector<uint64_t> actors(n);
    for (unsigned j = 0; j < n; ++j) {
        unsigned h;
        unsigned long long a;
        if (!read_key(&keys[size_t(j) * 64]) || std::scanf("%u %llu", &h, &a) != 2) return 2;
        has[j] = uint8_t(h);
        actors[j] = a;
    }
    const uint32_t n_slots = fs_slots_for(n);
    // exactly the sizes the contract names, each in an allocation of its own: a sanitizer sees any index past them
    std::vector<FsSlot> slots(n_slots);
    std::vector<FsGroup> groups(n);
    std::vector<FsMember> members(n);
    std::vector<uint32_t> group_of(n);
    const uint32_t n_groups = fs_build(keys.data(), has.data(), actors.data(), n, slots.data(), n_slots, groups.data(), members.data(),
                                       group_of.data());
    const FsView view{slots.data(), groups.data(), members.data(), n_slots - 1, n_groups, n, 0};
    std::printf("%u %u\n", n_slots, n_groups);
    unsigned n_probes;
    if (std::scanf("%u", &n_probes) != 1) return 2;
    for (unsigned i = 0; i < n_probes; ++i) {
        uint8_t key[64];
        unsigned long long emitter;
        uint64_t w[8];
        if (!read_key(key) || std::scanf("%llu", &emitter) != 1) return 2;
        words_of(key, w);
        uint32_t compares = 0;
        const uint32_t g = fs_probe(view, w, &compares);
        std::printf("%d %u", g == kFsNone ? -1 : int(g), compares);
        if (g != kFsNone)
            for (uint32_t m = 0; m < groups[g].count; ++m) {
                const FsMember& mem = members[groups[g].first + m];
                if (!mem.has_actor || mem.actor == emitter) std::printf(" %u", mem.spec);
            }
        std::printf("\n");
    }
    return 0;
}
