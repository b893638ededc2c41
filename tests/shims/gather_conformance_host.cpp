// TEST INFRASTRUCTURE.  Host half of the entity gather API conformance check (see
// gather_conformance.inl): plain host C++, as a simulator's Manager is.
#define GATHERCONF_NAME gatherconf_host
#include "gather_conformance.inl"
