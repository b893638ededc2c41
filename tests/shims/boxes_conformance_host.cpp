// TEST INFRASTRUCTURE.  Host half of the box query API conformance check (see
// boxes_conformance.inl): plain host C++, as a simulator's Manager is.
#define BOXESCONF_NAME boxesconf_host
#include "boxes_conformance.inl"
