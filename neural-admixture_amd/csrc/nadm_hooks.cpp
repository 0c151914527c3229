// The test hooks: process-wide switches that override a launch rule of the passes' host unit (nadm_decode_slices, nadm_encode_slices, the
// choice of the MLP kernels read them through the getters below).  This is the only unit that sees NADM_TEST_HOOKS: csrc/build.sh compiles it
// without the macro for libnadm.so -- no setter exists, every getter returns 0 -- and with it for libnadm_testhooks.so, which the
// tests that need a hook load in a child process (tests/conftest.py: in_hook_build).  Both libraries link the same kernel objects.
#include "nadm_host_rules.h"

#ifdef NADM_TEST_HOOKS
#include <atomic>

static std::atomic<int> g_force_slices{0};
static std::atomic<int> g_force_p3_slices{0};
static int g_force_generic_mlp = 0;
extern "C" void nadm_test_force_slices(int32_t n) { g_force_slices.store(n < 0 ? 0 : (n > NADM_MAX_P2_SLICES ? NADM_MAX_P2_SLICES : n)); }
extern "C" void nadm_test_force_p3_slices(int32_t n) { g_force_p3_slices.store(n < 0 ? 0 : (n > NADM_MAX_P2_SLICES ? NADM_MAX_P2_SLICES : n)); }
extern "C" void nadm_test_force_generic_mlp(int32_t on) { g_force_generic_mlp = on != 0; }

int nadm::hook_p2_slices() { return g_force_slices.load(); }
int nadm::hook_p3_slices() { return g_force_p3_slices.load(); }
int nadm::hook_generic_mlp() { return g_force_generic_mlp; }
#else
int nadm::hook_p2_slices() { return 0; }
int nadm::hook_p3_slices() { return 0; }
int nadm::hook_generic_mlp() { return 0; }
#endif
