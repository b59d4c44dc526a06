// Development: prints every field of the switch table (csrc/common.h: Switches) as a development build fills it -- with none of its
// environment variables set, then once per variable with that variable alone set (a process of its own each time: the table is filled
// once per process) -- and for each variable the fields that moved.  The check of the table: every default is the literal the code had
// before the table, and every name moves its own field and no other.
//
//   hipcc -std=c++17 -O1 -DAVMOE_DEV tests/dev/switches_dump.cpp avmoe_amd/csrc/common.cpp -o switches_dump && ./switches_dump
//   (+ -fsanitize=address,undefined for the sanitizer run)
//
// Host only: no GPU, nothing but common.cpp is linked.  Exit status 1 when a variable moves no field, another field, or more than one.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../avmoe_amd/csrc/common.h"

using namespace avmoe;

struct Var { const char* env; const char* field; const char* value; };
static const std::vector<Var> vars = {
  {"AVMOE_TOKPAIR2_FORCE", "hook_mask", "1"}, {"AVMOE_DPAIR_FORCE", "hook_mask", "1"}, {"AVMOE_HOP1S_FORCE", "hook_mask", "1"},
  {"AVMOE_KFS_FORCE", "hook_mask", "1"}, {"AVMOE_KFS_OFF", "hook_mask", "1"}, {"AVMOE_NXN_CHUNK", "nxn_chunk", "3"},
#define X(name, env) {env, #name, "1"},
  AVMOE_DEV_FLAGS(X)
#undef X
#define X(type, name, env, dflt, nonempty) {env, #name, "3"},
  AVMOE_DEV_NUMS(X)
#undef X
#define X(name, env) {env, #name, "2,3"},
  AVMOE_DEV_TEXTS(X)
#undef X
};

static void print_table() {
  const Switches& s = switches();
  printf("hook_mask=%u\nnxn_chunk=%d\n", s.hook_mask.load(), s.nxn_chunk.load());
#define X(name, env) printf(#name "=%d\n", (int)s.name);
  AVMOE_DEV_FLAGS(X)
#undef X
#define X(type, name, env, dflt, nonempty) printf(#name "=%ld\n", (long)s.name);
  AVMOE_DEV_NUMS(X)
#undef X
#define X(name, env) printf(#name "=%s\n", s.name ? s.name : "(unset)");
  AVMOE_DEV_TEXTS(X)
#undef X
}

static std::vector<std::pair<std::string, std::string>> run_self(const char* self, const char* env, const char* value) {
  std::string cmd;
  if (env) cmd = std::string(env) + "=" + value + " ";
  cmd += std::string("'") + self + "' --print";
  std::vector<std::pair<std::string, std::string>> out;
  FILE* p = popen(cmd.c_str(), "r");
  char line[256];
  while (p && fgets(line, sizeof line, p)) {
    line[strcspn(line, "\n")] = 0;
    if (char* eq = strchr(line, '=')) { *eq = 0; out.emplace_back(line, eq + 1); }
  }
  if (p) pclose(p);
  return out;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--print")) { print_table(); return 0; }
  for (const Var& v : vars) unsetenv(v.env);
  const auto base = run_self(argv[0], nullptr, nullptr);
  printf("nothing set (%zu fields)\n", base.size());
  for (const auto& kv : base) printf("  %s=%s\n", kv.first.c_str(), kv.second.c_str());
  int bad = base.size() != 2 + vars.size() - 6;            // (the six hook variables share two fields)
  for (const Var& v : vars) {
    const auto got = run_self(argv[0], v.env, v.value);
    printf("%s=%s\n", v.env, v.value);
    int moved = 0, own = 0;
    for (size_t i = 0; i < got.size() && i < base.size(); ++i) {
      if (got[i].second == base[i].second) continue;
      printf("  %s: %s -> %s\n", got[i].first.c_str(), base[i].second.c_str(), got[i].second.c_str());
      ++moved; own += got[i].first == v.field;
    }
    if (got.size() != base.size() || moved != 1 || own != 1) { printf("  ^^^ WRONG: expected %s alone to move\n", v.field); bad = 1; }
  }
  printf(bad ? "FAILED\n" : "every name moves its own field and no other\n");
  return bad;
}
