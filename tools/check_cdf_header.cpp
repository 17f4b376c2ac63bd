// check_cdf_header.cpp -- the NetCDF classic header parser and the variable checker of extpom_amd/csrc/cdf_io.hpp against damaged headers,
// as a stand-alone host program meant to be built with sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iextpom_amd/csrc -o check_cdf_header tools/check_cdf_header.cpp
//   ./check_cdf_header FILE.nc...
// For every file: the header as it stands must parse and every variable must pass the checker when asked for its own lengths.  Then a
// scratch copy is damaged: every 4-byte word of the header overwritten by 0xffffffff in turn (counts, tags, dimension ids, lengths, types,
// offsets), and the file cut to every prefix of its header.  A refusal is fine -- the count is printed -- a crash or a sanitizer report is
// the failure.  Exit status 0: every file went through; 1: a file could not be read, or an intact header was refused.
#define CDF_IO_HOST_ONLY
#include "cdf_io.hpp"

#include <fcntl.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>

// every variable of H asked for as each reader would: its own lengths (which an intact file passes) and lengths it does not have
static int check_all(const RHeader &H, uint64_t fsize, bool must_pass) {
  int refused = 0;
  for (const RVar &v : H.vars) {
    std::vector<uint64_t> own, inner;
    for (size_t d = 0; d < v.dimids.size(); d++) { own.push_back(H.dimlen[v.dimids[d]]); if (d) inner.push_back(own.back()); }
    const bool rec = !own.empty() && own[0] == 0;
    const RVar *out = NULL;
    const VarWant fits = rec ? VarWant::record(NC_NUMBER | 4u, inner, 1) : VarWant::fixed(NC_NUMBER | 4u, own);
    const std::string why = check_var(H, fsize, v.name.c_str(), fits, &out);
    if (!why.empty()) { refused++; if (must_pass) { fprintf(stderr, "an intact header was refused: %s\n", why.c_str()); return -1; } }
    std::vector<uint64_t> other = own;
    other.push_back(3);
    const VarWant wants[] = {VarWant::fixed(NC_ONLY_DOUBLE, own), VarWant::fixed(NC_REAL, own, VarWant::AT_LEAST), VarWant::fixed(NC_NUMBER, {}, VarWant::ONE_VALUE),
                             VarWant::record(NC_REAL, inner, 12), VarWant::shape(NC_REAL, other, "([records, ]"), VarWant::fixed(NC_NUMBER, other, VarWant::AT_LEAST)};
    for (const VarWant &w : wants) if (!check_var(H, fsize, v.name.c_str(), w, &out).empty()) refused++;
  }
  const RVar *out = NULL;
  if (!check_var(H, fsize, "no such variable", VarWant::fixed(NC_REAL, {}), &out).empty()) refused++;
  return refused;
}
// 0 = parsed (its variables checked), 1 = refused
static int one(int fd, uint64_t fsize, long &refusals) {
  RHeader H;
  std::string what;
  if (read_header(fd, fsize, H, what) < 0) { refusals++; return 1; }
  refusals += check_all(H, fsize, false);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s FILE.nc...\n", argv[0]); return 2; }
  for (int a = 1; a < argc; a++) {
    const int src = open(argv[a], O_RDONLY);
    struct stat sb;
    if (src < 0 || fstat(src, &sb)) { fprintf(stderr, "cannot open %s\n", argv[a]); return 1; }
    std::vector<unsigned char> all((size_t)sb.st_size);
    if (!all.empty() && pread_all(src, all.data(), all.size(), 0)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
    RHeader H;
    std::string what;
    if (read_header(src, all.size(), H, what) < 0) { fprintf(stderr, "%s: %s\n", argv[a], what.c_str()); return 1; }
    (void)close(src);
    if (check_all(H, all.size(), true) < 0) return 1;
    uint64_t hlen = all.size();                                  // the header ends where the first variable begins
    for (const RVar &v : H.vars) if (v.begin < hlen) hlen = v.begin;
    char tmpl[] = "/tmp/check_cdf_header_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0 || pwrite(fd, all.data(), all.size(), 0) != (ssize_t)all.size()) { fprintf(stderr, "no scratch file\n"); return 1; }
    (void)unlink(tmpl);
    long words = 0, prefixes = 0, parsed = 0, refusals = 0;
    const unsigned char ff[4] = {0xff, 0xff, 0xff, 0xff};
    for (uint64_t at = 0; at + 4 <= hlen; at += 4, words++) {    // one damaged word at a time
      if (pwrite(fd, ff, 4, (off_t)at) != 4) return 1;
      parsed += !one(fd, all.size(), refusals);
      if (pwrite(fd, all.data() + at, 4, (off_t)at) != 4) return 1;
    }
    for (uint64_t n = hlen; n-- > 0; prefixes++) {               // every prefix of the header, longest first
      if (ftruncate(fd, (off_t)n)) return 1;
      parsed += !one(fd, n, refusals);
    }
    (void)close(fd);
    printf("%s: %zu variables, header %llu bytes: %ld damaged words, %ld prefixes, %ld still parsed, %ld refusals\n", argv[a], H.vars.size(),
           (unsigned long long)hlen, words, prefixes, parsed, refusals);
  }
  printf("CDF-HEADER-OK\n");
  return 0;
}
