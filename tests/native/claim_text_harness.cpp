// tests/native/claim_text_harness.cpp — csrc/kernels/claim_text_dev.h compiled as host C++ (tests/test_claim_text_host.py).
// Reads one case per line on stdin and prints what the primitives give, the front-to-back form and the character-at-k
// form side by side:
//     u <decimal u64>      →  <dec_len> <put_u64> <dec_char_u64 …>
//     i <decimal i64>      →  <dec_len> <put_i64> <dec_char_i64 …>
//     x <hex bytes | ->    →  <put_hex0x> 0x<hex_char …>
//     c <80 hex digits>    →  <slot_cid_len> [<cid_str_len> <put_cid_str> <cid_str_char …>]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../ipc-filecoin-proofs_amd/csrc/kernels/claim_text_dev.h"

using namespace ipcfp::claimtext;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoul(s.substr(i, 2), nullptr, 16)));
    return out;
}

int main() {
    std::string kind, arg;
    while (std::cin >> kind >> arg) {
        if (kind == "u") {
            const uint64_t v = std::strtoull(arg.c_str(), nullptr, 10);
            std::vector<uint8_t> buf(dec_len_u64(v));  // exactly the length: a byte too many is the sanitizer's to find
            const uint32_t n = put_u64(buf.data(), v);
            std::string a(buf.begin(), buf.begin() + n), b;
            for (uint32_t k = 0; k < n; ++k) b.push_back(char(dec_char_u64(v, n, k)));
            std::cout << dec_len_u64(v) << ' ' << a << ' ' << b << '\n';
        } else if (kind == "i") {
            const int64_t v = int64_t(std::strtoll(arg.c_str(), nullptr, 10));
            std::vector<uint8_t> buf(dec_len_i64(v));
            const uint32_t n = put_i64(buf.data(), v);
            std::string a(buf.begin(), buf.begin() + n), b;
            for (uint32_t k = 0; k < n; ++k) b.push_back(char(dec_char_i64(v, n, k)));
            std::cout << dec_len_i64(v) << ' ' << a << ' ' << b << '\n';
        } else if (kind == "x") {
            const std::vector<uint8_t> p = unhex(arg);
            std::vector<uint8_t> buf(2 + 2 * p.size());
            const uint32_t n = put_hex0x(buf.data(), p.data(), uint32_t(p.size()));
            std::string a(buf.begin(), buf.begin() + n), b = "0x";
            for (uint64_t k = 0; k < 2 * p.size(); ++k) b.push_back(char(hex_char(p.data(), k)));
            std::cout << a << ' ' << b << '\n';
        } else if (kind == "c") {
            const std::vector<uint8_t> slot = unhex(arg);
            if (slot.size() != kSlotBytes) return 2;
            const int len = slot_cid_len(slot.data());
            std::cout << len;
            if (len > 0) {
                // the CID alone in a buffer of its own length: reading past it is the sanitizer's to find
                const std::vector<uint8_t> cid(slot.begin(), slot.begin() + len);
                const uint32_t sl = cid_str_len(cid.data(), uint32_t(len));
                std::vector<uint8_t> buf(sl);
                const uint32_t n = put_cid_str(buf.data(), cid.data(), uint32_t(len));
                std::string a(buf.begin(), buf.begin() + n), b;
                for (uint32_t k = 0; k < sl; ++k) b.push_back(char(cid_str_char(cid.data(), uint32_t(len), k)));
                std::cout << ' ' << sl << ' ' << a << ' ' << b;
            }
            std::cout << '\n';
        } else {
            return 2;
        }
    }
    return 0;
}
