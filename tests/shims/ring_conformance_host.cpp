// TEST INFRASTRUCTURE.  Host half of the ring API conformance check (see
// ring_conformance.inl): plain host C++, as a simulator's Manager is.
#define RINGCONF_NAME ringconf_host
#include "ring_conformance.inl"
