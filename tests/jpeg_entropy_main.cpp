// Stand-alone driver of the host stage (handobjectconsist_amd/csrc/jpeg_entropy.hpp) for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I handobjectconsist_amd/csrc
//       tests/jpeg_entropy_main.cpp -o jpeg_entropy_main && ./jpeg_entropy_main file.jpg ...
// For every file: the parser + entropy decoder over the whole file (must succeed), over EVERY prefix of it, and over copies
// with single bytes overwritten from a seeded generator.  Every input is copied into a heap block of exactly its length
// and the packed frame into one of exactly its size, so a read or write one byte outside either is a sanitizer report.
// Exit status 0: no report, the whole file decoded, and a decode of the same bytes twice gave the same packed frame.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_entropy.hpp"

static int run(const uint8_t* bytes, size_t len, std::vector<uint8_t>* keep) {
    uint8_t* data = static_cast<uint8_t*>(malloc(len ? len : 1));  // exactly len bytes: no slack behind the stream
    memcpy(data, bytes, len);
    mrjpeg::JeStream s;
    int rc = mrjpeg::je_parse(data, (int64_t)len, s);
    if (rc == mrjpeg::JE_OK) {
        const int64_t need = mrjpeg::je_packed_bytes(s.g.width, s.g.height, s.g.ncomp, s.g.hl, s.g.vl);
        if (need < mrjpeg::JE_HEADER_BYTES || need > (int64_t)1 << 22) {  // (a mutated size field: up to 4 MB is decoded)
            free(data);
            return need < 0 ? 1000 : mrjpeg::JE_NOTIMPL;
        }
        uint8_t* packed = static_cast<uint8_t*>(malloc((size_t)need));
        rc = mrjpeg::je_decode(data, (int64_t)len, s, packed, need);
        if (keep && rc == mrjpeg::JE_OK) keep->assign(packed, packed + need);
        free(packed);
    }
    free(data);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t buf[4096];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
        std::vector<uint8_t> first, second;
        if (run(file.data(), file.size(), &first) != mrjpeg::JE_OK || run(file.data(), file.size(), &second) != mrjpeg::JE_OK ||
            first != second || first.empty()) {
            fprintf(stderr, "%s: the whole file does not decode (or not twice to the same frame)\n", argv[a]);
            return 1;
        }
        long counts[3] = {0, 0, 0};  // ok, bad argument, not implemented
        for (size_t n = 0; n < file.size(); n++) {
            const int rc = run(file.data(), n, nullptr);
            if (rc < -2 || rc > 0) return 1;
            counts[-rc]++;
        }
        uint64_t state = 0x9E3779B97F4A7C15ull ^ file.size();
        const int trials = 4000;
        std::vector<uint8_t> copy;
        for (int t = 0; t < trials; t++) {
            copy = file;
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const int hits = 1 + (int)((state >> 60) & 3);
            for (int h = 0; h < hits; h++) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                copy[(size_t)((state >> 33) % file.size())] = (uint8_t)(state >> 20);
            }
            const int rc = run(copy.data(), copy.size(), nullptr);
            if (rc < -2 || rc > 0) return 1;
            counts[-rc]++;
        }
        printf("%s: %zu bytes, %zu prefixes + %d mutations: %ld ok, %ld bad argument, %ld not implemented\n", argv[a],
               file.size(), file.size(), trials, counts[0], counts[1], counts[2]);
    }
    return 0;
}
