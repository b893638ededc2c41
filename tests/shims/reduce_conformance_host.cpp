// TEST INFRASTRUCTURE.  Host half of the world reduce API conformance check (see
// reduce_conformance.inl): plain host C++, as a simulator's Manager is.
#define REDUCECONF_NAME reduceconf_host
#include "reduce_conformance.inl"
