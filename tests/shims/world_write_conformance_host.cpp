// TEST INFRASTRUCTURE.  Host half of the world write API conformance check (see
// world_write_conformance.inl): plain host C++, as a simulator's Manager is.
#define WRITECONF_NAME writeconf_host
#include "world_write_conformance.inl"
